"""The selective scan (rlx_ssm_scan_f32) forward and forward + backward at 1 / 2 / 4 / 8 time chunks per workgroup, the causal conv
(rlx_ssm_conv_f32) and one Mamba2 block stack (rlx_mamba2_f32) forward and forward + backward at the reference's default minibatch
-- 256 environments of 128 tokens, d_model 128, expand 2, state 8, conv 4, one layer, a done rate of about 1/100 -- on
tools/ens_bench.py's event timer.  Measurement only: prints one JSON line, no pass / fail.  The largest difference of g and d_u
between chunk count 1 and every other count is printed so that a wrong split cannot post a time.

    python tools/ssm_bench.py [--envs 256] [--tokens 128] [--d_model 128] [--expand 2] [--state 8] [--conv 4] [--layers 1]
                              [--warmup 5] [--iters 50]
"""
import argparse
import json

import torch

from ens_bench import timed
from rlx_amd.hip import Ctx, mamba2_desc, mamba2_param_count


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("envs", 256), ("tokens", 128), ("d_model", 128), ("expand", 2), ("state", 8), ("conv", 4), ("layers", 1),
                          ("warmup", 5), ("iters", 50)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx = torch.device("cuda:0"), Ctx(0)
    g = torch.Generator(device="cpu").manual_seed(0)
    S, T, d, N, K, Ly = a.envs, a.tokens, a.d_model, a.state, a.conv, a.layers
    I, M = d * a.expand, S * T
    X = I + 2 * N
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    e = lambda *s: torch.empty(*s, device=dev)
    done = (torch.rand(S, T, generator=g) < 0.01).to(torch.uint8).to(dev)
    res = {"shape": {"S": S, "T": T, "d_model": d, "I": I, "N": N, "K": K, "layers": Ly, "rows": M, "done_rate": round(float(done.float().mean()), 4)}}

    # scan: algorithmic HBM bytes -- forward reads u, xp, z and writes g (+ the checkpoints with a backward); the backward reads u, xp,
    # z, d g and the checkpoints and writes d u, d xp, d z
    u, xp, proj, d_g = r(M, I), r(M, X), r(M, 2 * I), r(M, I)
    dtb, Alog, D = r(I) - 4.0, torch.log(torch.arange(1, N + 1.0))[None].repeat(I, 1).to(dev) + 0.1 * r(I, N), 1 + 0.1 * r(I)
    h0, gout, hT = r(S, I, N), e(M, I), e(S, I, N)
    grads = dict(d_u=e(M, I), d_xp=e(M, X), d_proj=e(M, 2 * I), d_dt_bias=e(I), d_A_log=e(I, N), d_D=e(I))
    ck = 4 * S * ((T + 15) // 16) * I * N
    fwd_b, bwd_b = 4 * M * (3 * I + X), 4 * M * (4 * I + X + 2 * I + X) + ck
    base = None
    for nc in (1, 2, 4, 8):
        f = lambda: ctx.ssm_scan(u, xp, proj, done, dtb, Alog, D, gout, h0, hT, n_chunks=nc)
        fb = lambda: ctx.ssm_scan(u, xp, proj, done, dtb, Alog, D, gout, h0, hT, d_g=d_g, n_chunks=nc, **grads)
        res[f"scan_fwd_us_c{nc}"] = round(1e3 * timed(f, a.warmup, a.iters), 1)
        res[f"scan_fwd_bwd_us_c{nc}"] = round(1e3 * timed(fb, a.warmup, a.iters), 1)
        res[f"scan_fwd_GBps_c{nc}"] = round(fwd_b / res[f"scan_fwd_us_c{nc}"] / 1e3, 1)
        res[f"scan_fwd_bwd_GBps_c{nc}"] = round((fwd_b + ck + bwd_b) / res[f"scan_fwd_bwd_us_c{nc}"] / 1e3, 1)
        cur = (gout.clone(), grads["d_u"].clone())
        base = base or cur
        res[f"max_abs_diff_vs_c1_c{nc}"] = max(float((x - y).abs().max()) for x, y in zip(cur, base))

    cw, cb, c0, uo, cT = 0.5 * r(K, I), 0.1 * r(I), r(S, K - 1, I), e(M, I), e(S, K - 1, I)
    cg = dict(d_u=d_g, d_proj=grads["d_proj"], d_conv_w=e(K, I), d_conv_b=e(I))
    res["conv_fwd_us"] = round(1e3 * timed(lambda: ctx.ssm_conv(proj, done, cw, cb, uo, c0, cT), a.warmup, a.iters), 1)
    res["conv_fwd_bwd_us"] = round(1e3 * timed(lambda: ctx.ssm_conv(proj, done, cw, cb, uo, c0, cT, **cg), a.warmup, a.iters), 1)

    desc = mamba2_desc(d, a.expand, N, K, Ly)
    parts = []
    for _ in range(Ly):
        for shape in ((d,), (d,), (d, 2 * I), (2 * I,), (K, I), (I,), (I, X), (X,), (I,), (I, N), (I,), (I, d), (d,)):
            parts.append((torch.randn(shape, generator=g) / shape[0] ** 0.5 if len(shape) == 2 else torch.zeros(shape)).reshape(-1))
        parts[-13] += 1.0                                                                   # ln scale
        parts[-5] -= 4.0                                                                    # dt_bias: softplus^-1 of about 0.02
        parts[-4] = torch.log(torch.arange(1, N + 1.0))[None].repeat(I, 1).reshape(-1)      # A_log
        parts[-3] += 1.0                                                                    # D
    params = torch.cat(parts).to(dev)
    assert params.numel() == mamba2_param_count(desc)
    x, d_out, H0, C0 = r(M, d), r(M, d), r(S, Ly, I, N), r(S, Ly, K - 1, I)
    out, HT, CT, dx, gr = e(M, d), e(S, Ly, I, N), e(S, Ly, K - 1, I), e(M, d), torch.empty_like(params)
    res["block_fwd_us"] = round(1e3 * timed(lambda: ctx.mamba2(desc, params, x, done, out, H0, C0, HT, CT), a.warmup, a.iters), 1)
    res["block_fwd_bwd_us"] = round(1e3 * timed(lambda: ctx.mamba2(desc, params, x, done, out, H0, C0, HT, CT, d_out, gr, dx), a.warmup,
                                                a.iters), 1)
    res["block_finite"] = bool(torch.isfinite(out).all() and torch.isfinite(gr).all() and torch.isfinite(dx).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
