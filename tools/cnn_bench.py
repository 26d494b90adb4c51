"""The convolutional torso (rlx_cnn_net_f32) at the reference shape -- 4 x 84 x 84 uint8, Conv(32, 8, 4) -> Conv(64, 4, 2) ->
Conv(64, 3, 1) -> Dense(512) -> Dense(6 x 51) -- forward and forward + backward on tools/ens_bench.py's event timer, beside torch's
own conv2d / linear on the same device and tensors.  Batches: dqn's default_config.py batch_size = 32 (norm 0) and pqn's minibatch,
nr_envs x nr_steps / nr_minibatches = 1 x 32 / 4 = 8 (norm 1), and 1024 images of both (pqn with 128 environments).  The library
and torch alternate, twice each (the second figure is kept), and a timed window is --iters calls at 1024 images and eight times
as many at the small batches: some 0.3 s and more of device time per window.  Measurement
only: one JSON line per run, no pass / fail; the largest difference of `out` and of the gradients between the library and torch is
printed so that a wrong result cannot post a time.

    python tools/cnn_bench.py [--warmup 5] [--iters 100] [--runs 2] [--rows 0] [--eager 1] [--small-m 0]
                              (--rows M --eager 0: one batch, library kernels only -- for a kernel trace;
                               --small-m 1: the option gemm_small_m, the hidden Dense on the split-K kernel of gemm_sk.hip)
"""
import argparse
import json

import torch
import torch.nn.functional as F

from ens_bench import timed
from rlx_amd.hip import Ctx, cnn_desc, cnn_param_count

CONVS, HIDDEN, OUT, EPS = ((32, 8, 4), (64, 4, 2), (64, 3, 1)), 512, 6 * 51, 1e-6
BATCHES = ((32, 0), (8, 1), (1024, 0), (1024, 1))


def ln(z, g, b):
    mean = z.mean(-1, keepdim=True)
    var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    return (z - mean) * torch.rsqrt(var + EPS) * g + b


def shapes(norm):
    out, ci, hw = [], 4, 84
    for co, k, s in CONVS:
        out += [(k, k, ci, co), (co,)] + [(co,)] * (2 * norm)
        ci, hw = co, (hw - k) // s + 1
    return out + [(hw * hw * ci, HIDDEN), (HIDDEN,)] + [(HIDDEN,)] * (2 * norm) + [(HIDDEN, OUT), (OUT,)]


def views(p, norm):
    out, off = [], 0
    for s in shapes(norm):
        n = torch.Size(s).numel()
        out.append(p[off:off + n].view(s))
        off += n
    return out


def eager(p, x, norm):
    w, h = views(p, norm), x.float() / 255
    per = 2 + 2 * norm
    for l, (co, k, s) in enumerate(CONVS):
        W, b = w[per * l], w[per * l + 1]
        z = F.conv2d(h, W.permute(3, 2, 0, 1), b, stride=s)
        h = torch.relu(ln(z.permute(0, 2, 3, 1), w[per * l + 2], w[per * l + 3]).permute(0, 3, 1, 2)) if norm else torch.relu(z)
    d = w[per * len(CONVS):]
    z = h.permute(0, 2, 3, 1).reshape(x.shape[0], -1) @ d[0] + d[1]
    return torch.relu(ln(z, d[2], d[3]) if norm else z) @ d[-2] + d[-1]


def one_run(a, ctx, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {}
    for M, norm in (((a.rows, 0), (a.rows, 1)) if a.rows else BATCHES):
        parts = []
        for s in shapes(norm):
            w = torch.randn(s, generator=g)
            parts.append((w * (2.0 / torch.Size(s[:-1]).numel()) ** 0.5 if len(s) > 1 else 0.1 * torch.tanh(w)).reshape(-1))
        params = torch.cat(parts)
        if norm:      # LayerNorm scales around 1: the third entry of every (W, b, g, be) group
            for i, v in enumerate(views(params, norm)[:-2]):
                if i % 4 == 2:
                    v += 1.0
        params = params.to(dev)
        desc = cnn_desc(OUT, norm=norm)
        assert params.numel() == cnn_param_count(desc)
        k = f"m{M}_norm{norm}"
        x = torch.randint(0, 256, (M, 4, 84, 84), generator=g, dtype=torch.uint8).to(dev)
        d_out, out, grads = torch.randn(M, OUT, generator=g).to(dev), torch.empty(M, OUT, device=dev), torch.empty_like(params)
        t = lambda f: round(1e3 * timed(f, a.warmup, a.iters * (8 if M <= 32 else 1)), 1)
        pe = params.clone().requires_grad_()

        def eager_fb():
            pe.grad = None
            eager(pe, x, norm).backward(d_out)

        def eager_f():
            with torch.no_grad():
                return eager(params, x, norm)

        for _ in range(2):      # the two sides alternate
            res[f"fwd_us_{k}"] = t(lambda: ctx.cnn_net(desc, params, x, out))
            if a.eager:
                res[f"eager_fwd_us_{k}"] = t(eager_f)
            res[f"fwd_bwd_us_{k}"] = t(lambda: ctx.cnn_net(desc, params, x, out, d_out, grads))
            if a.eager:
                res[f"eager_fwd_bwd_us_{k}"] = t(eager_fb)
        res[f"finite_{k}"] = bool(torch.isfinite(out).all() and torch.isfinite(grads).all())
        if a.eager:
            res[f"max_abs_diff_out_{k}"] = float((eager_f() - out).abs().max())
            res[f"max_rel_diff_grads_{k}"] = max(float((e - l).abs().max() / e.abs().max()) for e, l in zip(views(pe.grad, norm), views(grads, norm)))
    return res


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("warmup", 5), ("iters", 100), ("runs", 2), ("rows", 0), ("eager", 1), ("small-m", 0)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx = torch.device("cuda:0"), Ctx(0)
    ctx.set_option("gemm_small_m", a.small_m)
    for _ in range(a.runs):
        print(json.dumps(one_run(a, ctx, dev)), flush=True)


if __name__ == "__main__":
    main()
