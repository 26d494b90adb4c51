"""BroNet (rlx_bro_net_f32) forward on both routes (fwd_path 1 layered, 2 fused) side by side, forward + backward on the layered
route, and BRO's quantile critic loss (rlx_bro_quantile_loss_f32) at (128, 100) -- on tools/ens_bench.py's event timer, beside a
torch eager implementation of the same formulas on the same tensors.  Two shapes: the reference's critic (in_dim 23, hidden 512,
2 blocks, out_dim 100) and its policy trunk (hidden 256, 1 block, no output layer).  Measurement only: prints one JSON line per
run, no pass / fail; the largest difference of `out` between each route and eager is printed so that a wrong result cannot post a time.

    python tools/bro_bench.py [--warmup 5] [--iters 50] [--runs 2] [--rows 0] [--eager 1]
                              (--rows M --eager 0: one row count, library kernels only -- for a kernel trace)
"""
import argparse
import json

import torch

from ens_bench import timed
from rlx_amd.hip import Ctx, bro_desc, bro_param_count

SHAPES = {"critic": (23, 512, 2, 100), "policy": (23, 256, 1, 0)}
ROWS = (128, 256, 1024, 4096, 32768)
EPS = 1e-6


def ln(z, g, b):
    mean = z.mean(-1, keepdim=True)
    var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    return (z - mean) * torch.rsqrt(var + EPS) * g + b


def one_run(a, ctx, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {}
    for tag, (I, H, nb, O) in SHAPES.items():
        shapes = [(I, H)] + [(H,)] * 3 + ([(H, H)] + [(H,)] * 3) * 2 * nb + ([(H, O), (O,)] if O else [])
        parts = []
        for i, s in enumerate(shapes):
            w = torch.randn(s, generator=g)
            scale_slot = i < 4 + 8 * nb and i % 4 == 2      # the g of every (W, b, g, be) group
            parts.append((w * (2.0 / s[0]) ** 0.5 if len(s) == 2 else (1.0 if scale_slot else 0.0) + 0.1 * torch.tanh(w)).reshape(-1))
        params = torch.cat(parts).to(dev)
        assert params.numel() == bro_param_count(bro_desc(I, H, nb, O))

        def views(p):
            out, off = [], 0
            for s in shapes:
                n = s[0] * (s[1] if len(s) == 2 else 1)
                out.append(p[off:off + n].view(s))
                off += n
            return out

        def eager(p, x):
            w = views(p)
            h = torch.relu(ln(x @ w[0] + w[1], w[2], w[3]))
            for b in range(nb):
                Wa, ba, ga, bea, Wb, bb, gb, beb = w[4 + 8 * b:12 + 8 * b]
                y = torch.relu(ln(h @ Wa + ba, ga, bea))
                h = ln(y @ Wb + bb, gb, beb) + h
            return h @ w[-2] + w[-1] if O else h

        t = lambda f: round(1e3 * timed(f, a.warmup, a.iters), 1)
        for M in ((a.rows,) if a.rows else ROWS):
            k = f"{tag}_m{M}"
            x, d_out = torch.randn(M, I, generator=g).to(dev), torch.randn(M, O or H, generator=g).to(dev)
            out, grads, dx = torch.empty(M, O or H, device=dev), torch.empty_like(params), torch.empty(M, I, device=dev)
            d1, d2 = bro_desc(I, H, nb, O, fwd_path=1), bro_desc(I, H, nb, O, fwd_path=2)
            for _ in range(2):      # the two routes alternate
                res[f"fwd_layered_us_{k}"] = t(lambda: ctx.bro_net(d1, params, x, out))
                res[f"fwd_fused_us_{k}"] = t(lambda: ctx.bro_net(d2, params, x, out))
            res[f"fwd_bwd_us_{k}"] = t(lambda: ctx.bro_net(d1, params, x, out, d_out, grads, dx))
            res[f"finite_{k}"] = bool(torch.isfinite(out).all() and torch.isfinite(grads).all() and torch.isfinite(dx).all())
            if a.eager:
                pe, xe = params.clone().requires_grad_(), x.clone().requires_grad_()

                def eager_fb():
                    pe.grad = xe.grad = None
                    eager(pe, xe).backward(d_out)

                with torch.no_grad():
                    res[f"eager_fwd_us_{k}"] = t(lambda: eager(params, x))
                    ref = eager(params, x)
                res[f"eager_fwd_bwd_us_{k}"] = t(eager_fb)
                for path, d in ((1, d1), (2, d2)):
                    ctx.bro_net(d, params, x, out)
                    res[f"max_abs_diff_out_path{path}_{k}"] = float((ref - out).abs().max())
                res[f"max_rel_diff_grads_{k}"] = max(float((e - l).abs().max() / e.abs().max()) for e, l in zip(views(pe.grad), views(grads)))

    B, N, gamma, pess, kappa = 128, 100, 0.99, 0.5, 1.0
    q1, q2, n1, n2 = (torch.randn(B, N, generator=g).to(dev) for _ in range(4))
    rew, term, nlp = torch.randn(B, generator=g).to(dev), (torch.rand(B, generator=g) < 0.1).float().to(dev), torch.randn(B, generator=g).to(dev)
    la = torch.tensor([-0.7], device=dev)
    dq1, dq2, loss = torch.empty_like(q1), torch.empty_like(q2), torch.empty(1, device=dev)
    res["qloss_us_b128_n100"] = round(1e3 * timed(lambda: ctx.bro_quantile_loss(q1, q2, n1, n2, rew, term, nlp, la, gamma, pess, kappa, dq1, dq2, loss),
                                                  a.warmup, a.iters), 1)
    if a.eager:
        tau = ((torch.arange(N, device=dev) + 0.5) / N)[None, :, None]
        e1, e2 = q1.clone().requires_grad_(), q2.clone().requires_grad_()

        def eager_loss():
            e1.grad = e2.grad = None
            nq = (n1 + n2) / 2 - pess * (n1 - n2).abs() / 2
            y = rew[:, None] + (gamma * (1 - term))[:, None] * (nq - (la.exp() * nlp)[:, None])
            tot = 0
            for q in (e1, e2):
                td = y[:, None, :] - q[:, :, None]
                hub = torch.where(td.abs() <= kappa, 0.5 * td ** 2, kappa * (td.abs() - 0.5 * kappa))
                tot = tot + ((tau - (td < 0).float()).abs() * hub / kappa).sum() / (B * N)
            tot.backward()
            return tot

        res["eager_qloss_us_b128_n100"] = round(1e3 * timed(eager_loss, a.warmup, a.iters), 1)
        res["qloss_rel_diff"] = abs(float(eager_loss()) - float(loss)) / abs(float(loss))
        res["qloss_max_abs_diff_dq"] = max(float((e1.grad - dq1).abs().max()), float((e2.grad - dq2).abs().max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("warmup", 5), ("iters", 50), ("runs", 2), ("rows", 0), ("eager", 1)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx = torch.device("cuda:0"), Ctx(0)
    for _ in range(a.runs):
        print(json.dumps(one_run(a, ctx, dev)), flush=True)


if __name__ == "__main__":
    main()
