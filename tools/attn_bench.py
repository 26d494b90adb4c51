"""One banded attention forward + backward (rlx_band_attn_f32) and one encoder forward + backward (rlx_tf_encoder_f32) at the
reference's default minibatch -- 256 environments of 15 + 128 tokens, d_model 128, 4 heads, dim_ff 512, 2 layers, window 16, a done
rate of about 1/100 -- on tools/ens_bench.py's event timer.  Beside the attention, torch.nn.functional.scaled_dot_product_attention
forward + backward on the same device with the dense boolean mask.  Measurement only: prints one JSON line, no pass / fail.  The
largest difference between the two attentions' outputs at valid rows is printed so that a wrong kernel cannot post a time.

    python tools/attn_bench.py [--envs 256] [--tokens 143] [--d_model 128] [--heads 4] [--ff 512] [--layers 2] [--window 16]
                               [--warmup 5] [--iters 50]
"""
import argparse
import json

import torch
import torch.nn.functional as F

from ens_bench import timed
from rlx_amd.hip import Ctx, tf_desc, tf_param_count


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("envs", 256), ("tokens", 143), ("d_model", 128), ("heads", 4), ("ff", 512), ("layers", 2), ("window", 16),
                          ("warmup", 5), ("iters", 50)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx = torch.device("cuda:0"), Ctx(0)
    g = torch.Generator(device="cpu").manual_seed(0)
    S, T, D, H, C = a.envs, a.tokens, a.d_model, a.heads, a.window
    M, hd = S * T, a.d_model // a.heads
    seg = (torch.rand(S, T, generator=g) < 0.01).cumsum(1).to(torch.int32)
    valid = (torch.arange(T)[None, :] >= torch.randint(0, C, (S, 1), generator=g)).to(torch.uint8)     # a fresh history's padding
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    keep = ((i - j >= 0) & (i - j < C))[None] & (seg[:, :, None] == seg[:, None, :]) & (valid[:, :, None] & valid[:, None, :]).bool()
    rows = valid.reshape(-1).bool().to(dev)
    qkv, d_out = torch.randn(M, 3 * D, generator=g).to(dev), torch.randn(M, D, generator=g).to(dev)
    seg_d, valid_d, keep_d = seg.to(dev), valid.to(dev), keep[:, None].to(dev)
    out, lse, dqkv = torch.empty(M, D, device=dev), torch.empty(M, H, device=dev), torch.empty(M, 3 * D, device=dev)
    res = {"shape": {"S": S, "T": T, "d_model": D, "nhead": H, "dim_ff": a.ff, "layers": a.layers, "window": C, "rows": M,
                     "valid_fraction": round(float(valid.float().mean()), 4)}}
    res["attn_fwd_us"] = round(1e3 * timed(lambda: ctx.band_attn(qkv, seg_d, valid_d, H, C, out, lse), a.warmup, a.iters), 1)
    res["attn_fwd_bwd_us"] = round(1e3 * timed(lambda: ctx.band_attn(qkv, seg_d, valid_d, H, C, out, lse, d_out, dqkv), a.warmup, a.iters), 1)
    # algorithmic HBM bytes: forward reads qkv and writes out + lse; the backward reads qkv, out, lse, d_out and writes dqkv
    fwd_b, bwd_b = 4 * M * (3 * D + D + H), 4 * M * (3 * D + D + H + D + 3 * D)
    res["attn_fwd_GBps"] = round(fwd_b / res["attn_fwd_us"] / 1e3, 1)
    res["attn_fwd_bwd_GBps"] = round((fwd_b + bwd_b) / res["attn_fwd_bwd_us"] / 1e3, 1)

    # torch: the same tensors as [S, H, T, hd] views of a leaf, the dense mask; rows that keep nothing get NaN there and are not compared
    x = qkv.reshape(S, T, 3, H, hd).permute(2, 0, 3, 1, 4).contiguous().requires_grad_()
    go = d_out.reshape(S, T, H, hd).permute(0, 2, 1, 3).contiguous()

    def sdpa(bwd):
        o = F.scaled_dot_product_attention(x[0], x[1], x[2], attn_mask=keep_d)
        if bwd:
            x.grad = None
            o.backward(go)
        return o
    res["sdpa_fwd_us"] = round(1e3 * timed(lambda: sdpa(False), a.warmup, a.iters), 1)
    res["sdpa_fwd_bwd_us"] = round(1e3 * timed(lambda: sdpa(True), a.warmup, a.iters), 1)
    o_t = sdpa(False).detach().permute(0, 2, 1, 3).reshape(M, D)
    res["max_abs_diff_vs_sdpa_valid_rows"] = float((o_t - out)[rows].abs().max())

    desc = tf_desc(D, H, a.ff, a.layers, C)
    parts = []
    for _ in range(a.layers):
        for shape in ((D,), (D,), (D, 3 * D), (3 * D,), (D, D), (D,), (D,), (D,), (D, a.ff), (a.ff,), (a.ff, D), (D,)):
            parts.append((torch.randn(shape, generator=g) / shape[0] ** 0.5 if len(shape) == 2 else torch.zeros(shape)).reshape(-1))
        parts[-12] += 1.0       # ln1 scale
        parts[-6] += 1.0        # ln2 scale
    params = torch.cat(parts).to(dev)
    assert params.numel() == tf_param_count(desc)
    xe = torch.randn(M, D, generator=g).to(dev)
    eo, dx, grads = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev), torch.empty_like(params)
    res["encoder_fwd_us"] = round(1e3 * timed(lambda: ctx.tf_encoder(desc, params, xe, seg_d, valid_d, eo), a.warmup, a.iters), 1)
    res["encoder_fwd_bwd_us"] = round(1e3 * timed(lambda: ctx.tf_encoder(desc, params, xe, seg_d, valid_d, eo, d_out, grads, dx), a.warmup,
                                                  a.iters), 1)
    res["encoder_finite"] = bool(torch.isfinite(eo[rows]).all() and torch.isfinite(grads).all() and torch.isfinite(dx).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
