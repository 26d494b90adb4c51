"""The hyperspherical network (rlx_hyper_net_f32) forward and forward + backward and the projection (rlx_hyper_project_f32) at the
reference's batch (256 rows) and at 32768 rows -- in_dim 23, hidden 512, two blocks, expansion 4 -- on tools/ens_bench.py's event
timer, beside a torch eager implementation of the same formulas (autograd for its backward, torch.no_grad for its projection) on the
same tensors.  Measurement only: prints one JSON line, no pass / fail; the largest difference of `out` and of the projected
parameters between the two is printed so that a wrong result cannot post a time.

    python tools/hyper_bench.py [--in_dim 23] [--hidden 512] [--blocks 2] [--expansion 4] [--warmup 5] [--iters 50]
                                [--rows 0] [--eager 1] [--small-m 0]
        (--rows M --eager 0: one shape, library kernels only -- for a kernel trace; --small-m 1: the option gemm_small_m, the blocks'
         products on the split-K kernel of gemm_sk.hip where its rule takes them)
"""
import argparse
import json

import torch

from ens_bench import timed
from rlx_amd.hip import Ctx, hyper_desc, hyper_param_count

EPS = 1e-8


def l2n(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(EPS)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("in_dim", 23), ("hidden", 512), ("blocks", 2), ("expansion", 4), ("warmup", 5), ("iters", 50), ("rows", 0),
                          ("eager", 1), ("small-m", 0)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx = torch.device("cuda:0"), Ctx(0)
    ctx.set_option("gemm_small_m", a.small_m)
    g = torch.Generator(device="cpu").manual_seed(0)
    I, H, X, nb = a.in_dim, a.hidden, a.hidden * a.expansion, a.blocks
    desc = hyper_desc(I, H, nb, a.expansion)
    cs, ca = desc.scaler_init / desc.scaler_scale, desc.alpha_init / desc.alpha_scale
    shapes = [(I + 1, H), (H,)] + [(H, X), (X,), (X, H), (H,)] * nb
    inits = [None, desc.scaler_scale] + [None, desc.scaler_scale / a.expansion ** 0.5, None, desc.alpha_scale] * nb
    parts = []
    for shape, init in zip(shapes, inits):
        w = torch.randn(shape, generator=g)
        parts.append((w / w.norm(dim=0, keepdim=True) if init is None else init * (1 + 0.1 * torch.tanh(w))).reshape(-1))
    params = torch.cat(parts).to(dev)
    assert params.numel() == hyper_param_count(desc)

    def views(p):
        out, off = [], 0
        for shape in shapes:
            n = shape[0] * (shape[1] if len(shape) == 2 else 1)
            out.append(p[off:off + n].view(shape))
            off += n
        return out

    def eager(p, x):
        w = views(p)
        h = l2n(w[1] * (cs * (l2n(torch.cat([x, x.new_full((x.shape[0], 1), desc.c_shift)], 1)) @ w[0])))
        for b in range(nb):
            W1, s1, W2, al = w[2 + 4 * b:6 + 4 * b]
            y = l2n((torch.relu(s1 * (cs * (h @ W1))) + EPS) @ W2)
            h = l2n(h + al * (ca * (y - h)))
        return h

    def eager_project(p):
        with torch.no_grad():
            for w in views(p):
                if w.dim() == 2:
                    w.div_(w.norm(dim=0, keepdim=True).clamp_min(EPS))

    res = {"shape": {"in_dim": I, "hidden": H, "X": X, "blocks": nb, "params": params.numel()}}
    for M in ((a.rows,) if a.rows else (256, 32768)):
        x, d_out = torch.randn(M, I, generator=g).to(dev), torch.randn(M, H, generator=g).to(dev)
        out, grads, dx = torch.empty(M, H, device=dev), torch.empty_like(params), torch.empty(M, I, device=dev)
        pe, xe = params.clone().requires_grad_(), x.clone().requires_grad_()

        def eager_fb():
            pe.grad = xe.grad = None
            eager(pe, xe).backward(d_out)

        t = lambda f: round(1e3 * timed(f, a.warmup, a.iters), 1)
        if a.eager:
            with torch.no_grad():
                res[f"eager_fwd_us_m{M}"] = t(lambda: eager(params, x))
        res[f"fwd_us_m{M}"] = t(lambda: ctx.hyper_net(desc, params, x, out))
        res[f"fwd_bwd_us_m{M}"] = t(lambda: ctx.hyper_net(desc, params, x, out, d_out, grads, dx))
        if a.eager:
            res[f"eager_fwd_bwd_us_m{M}"] = t(eager_fb)
            with torch.no_grad():
                res[f"max_abs_diff_out_m{M}"] = float((eager(params, x) - out).abs().max())
            res[f"max_abs_diff_grads_m{M}"] = float((pe.grad - grads).abs().max())
            # per tensor of the layout, relative to the tensor's largest entry (the Scaler gradients are sums of O(rows) terms)
            res[f"max_rel_diff_grads_m{M}"] = max(float((e - l).abs().max() / e.abs().max()) for e, l in zip(views(pe.grad), views(grads)))
        res[f"finite_m{M}"] = bool(torch.isfinite(out).all() and torch.isfinite(grads).all() and torch.isfinite(dx).all())

    p1, p2 = params * 1.5, params * 1.5
    res["project_us"] = round(1e3 * timed(lambda: ctx.hyper_project(desc, p1), a.warmup, a.iters), 1)
    if a.eager:
        res["eager_project_us"] = round(1e3 * timed(lambda: eager_project(p2), a.warmup, a.iters), 1)
        res["max_abs_diff_project"] = float((p1 - p2).abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
