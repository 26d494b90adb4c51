"""Time one AQE update (rlx_aqe_update_f32: G critic steps on G batches, then one policy step) at the reference's defaults --
ensemble 10, 2 heads per net, 4 of the 20 pooled target values dropped, 5 critic steps, hidden 256 -- at obs 376, act 17, for batches
of 256 and 4096 rows on one MI355X, and -- same shapes, same process -- G + 1 SAC updates (rlx_sac_update_f32, two scalar critics)
beside it: what the same number of optimizer rounds costs on the fused twin-critic path.  Prints one JSON line per configuration:
ms per call, calls / s and (AQE) critic steps / s.

    python tools/aqe_bench.py [--iters 20] [--warmup 3] [--only E,H,dropped,G,B] [--no-sac]

Launches per call: trace the tool twice with different --iters for one configuration and divide the difference of the kernel
counts by the difference of the iteration counts (everything outside the timed loop cancels), e.g.
    rocprofv3 --kernel-trace --output-format csv -d out2 -- python tools/aqe_bench.py --only 10,2,4,5,256 --no-sac --warmup 0 --iters 2
    rocprofv3 --kernel-trace --output-format csv -d out4 -- python tools/aqe_bench.py --only 10,2,4,5,256 --no-sac --warmup 0 --iters 4
    (rows of out4/*kernel_trace.csv - rows of out2/*kernel_trace.csv) / 2"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rl-x_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

O, A, W = 376, 17, 256


def lecun(rng, in_dim, hidden, out_dim):
    parts, d = [], in_dim
    for h in list(hidden) + [out_dim]:
        parts += [(np.clip(rng.standard_normal((d, h)), -2, 2) * np.sqrt(1.0 / d) / 0.87962566103423978).ravel(), np.zeros(h)]
        d = h
    return np.concatenate(parts).astype(np.float32)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="E,H,dropped,G,B: one AQE configuration")
    ap.add_argument("--no-sac", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import ACT_RELU, AqeHparams, Ctx, SacHparams, mlp_desc
    from rlx_amd.hip import lib as L
    dev = torch.device("cuda:0")
    ctx = Ctx(0)
    rng = np.random.default_rng(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    pd = mlp_desc(O, [W, W], 2 * A, ACT_RELU, False, False)
    qd1 = mlp_desc(O + A, [W, W], 1, ACT_RELU, False, False)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(10, 2, 4, 5, 256), (10, 2, 4, 5, 4096)]

    def state(E, H):
        pp = lecun(rng, O, [W, W], 2 * A)
        pp[-(W * 2 * A + 2 * A):] *= 0.1                       # std ~ 1: the tanh rarely saturates
        P = t(pp)
        Q = t(np.concatenate([lecun(rng, O + A, [W, W], H) for _ in range(E)]))
        return dict(P=P, pm=torch.zeros_like(P), pv=torch.zeros_like(P), Q=Q, qm=torch.zeros_like(Q), qv=torch.zeros_like(Q), QT=Q.clone(),
                    la=torch.zeros(1, device=dev), am=torch.zeros(1, device=dev), av=torch.zeros(1, device=dev))

    def batch(G, B):
        return (t(rng.standard_normal((G, B, O))), t(rng.standard_normal((G, B, O))), t(np.tanh(rng.standard_normal((G, B, A)))),
                t(rng.standard_normal((G, B))), t(rng.random((G, B)) < 0.1))

    def run_aqe(E, H, dropped, G, B):
        st, b, met = state(E, H), batch(G, B), torch.zeros(10, device=dev)
        qd = mlp_desc(O + A, [W, W], H, ACT_RELU, False, False)
        hp = AqeHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, H, dropped, G)
        box = dict(key=L.prng_key(0), q=0, pi=0)

        def fn():
            box["key"], box["q"], box["pi"] = ctx.aqe_update(pd, st["P"], st["pm"], st["pv"], qd, st["Q"], st["qm"], st["qv"], st["QT"], st["la"],
                                                             st["am"], st["av"], b, box["key"], box["q"], box["pi"], hp, met)

        ms = timed(fn, args.warmup, args.iters)
        assert torch.isfinite(met).all(), met
        row = {"what": "aqe_update", "critics": E, "heads": H, "dropped": dropped, "critic_steps": G, "batch": B, "ms": round(ms, 3),
               "calls_per_s": round(1000.0 / ms, 2), "critic_steps_per_s": round(1000.0 * G / ms, 1)}
        print(json.dumps(row), flush=True)

    def run_sac(n, B):
        st, b, met = state(2, 1), tuple(x[0] for x in batch(1, B)), torch.zeros(10, device=dev)
        hp = SacHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8)
        box = dict(key=L.prng_key(0), count=0)

        def fn():
            for _ in range(n):
                box["key"], box["count"] = ctx.sac_update(pd, st["P"], st["pm"], st["pv"], qd1, st["Q"], st["qm"], st["qv"], st["QT"], st["la"],
                                                          st["am"], st["av"], b, box["key"], box["count"], hp, met)

        ms = timed(fn, args.warmup, args.iters)
        assert torch.isfinite(met).all(), met
        print(json.dumps({"what": "%d_sac_updates" % n, "critics": 2, "batch": B, "ms": round(ms, 3), "ms_per_update": round(ms / n, 4)}),
              flush=True)

    for E, H, dropped, G, B in configs:
        run_aqe(E, H, dropped, G, B)
    if not args.no_sac:
        for G, B in sorted({(c[3], c[4]) for c in configs}):
            run_sac(G + 1, B)


if __name__ == "__main__":
    main()
