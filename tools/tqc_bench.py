"""Time one TQC update (rlx_tqc_update_f32) at obs 376, act 17, hidden 256, 25 atoms per net, 2 dropped, for ensembles of 2 and 5
critics and batches of 256 and 4096 rows on one MI355X, and -- same shapes, same process -- one SAC update (rlx_sac_update_f32, two
scalar critics) beside it.  Prints one JSON line per configuration: ms per update and updates / s.

    python tools/tqc_bench.py [--iters 200] [--warmup 20] [--only E,B] [--no-sac]

Launches per update: trace the tool twice with different --iters for one configuration and divide the difference of the kernel
counts by the difference of the iteration counts (everything outside the timed loop cancels), e.g.
    rocprofv3 --kernel-trace --output-format csv -d out20 -- python tools/tqc_bench.py --only 2,256 --no-sac --warmup 0 --iters 20
    rocprofv3 --kernel-trace --output-format csv -d out40 -- python tools/tqc_bench.py --only 2,256 --no-sac --warmup 0 --iters 40
    (rows of out40/*kernel_trace.csv - rows of out20/*kernel_trace.csv) / 20"""
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

O, A, H, N, DROPPED = 376, 17, 256, 25, 2


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="", help="E,B: one TQC configuration")
    ap.add_argument("--no-sac", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import ACT_RELU, Ctx, SacHparams, TqcHparams, mlp_desc
    from rlx_amd.hip import lib as L
    dev = torch.device("cuda:0")
    ctx = Ctx(0)
    rng = np.random.default_rng(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    pd = mlp_desc(O, [H, H], 2 * A, ACT_RELU, False, False)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(2, 256), (5, 256), (2, 4096), (5, 4096)]

    def run(kind, E, B):
        out_dim = N if kind == "tqc" else 1
        qd = mlp_desc(O + A, [H, H], out_dim, ACT_RELU, False, False)
        pp = lecun(rng, O, [H, H], 2 * A)
        pp[-(H * 2 * A + 2 * A):] *= 0.1                       # std ~ 1: the tanh rarely saturates
        P = t(pp)
        Q = t(np.concatenate([lecun(rng, O + A, [H, H], out_dim) for _ in range(E)]))
        st = dict(P=P, pm=torch.zeros_like(P), pv=torch.zeros_like(P), Q=Q, qm=torch.zeros_like(Q), qv=torch.zeros_like(Q), QT=Q.clone(),
                  la=torch.zeros(1, device=dev), am=torch.zeros(1, device=dev), av=torch.zeros(1, device=dev))
        batch = (t(rng.standard_normal((B, O))), t(rng.standard_normal((B, O))), t(np.tanh(rng.standard_normal((B, A)))),
                 t(rng.standard_normal(B)), t(rng.random(B) < 0.1))
        met = torch.zeros(10, device=dev)
        box = dict(key=L.prng_key(0), count=0)
        if kind == "tqc":
            hp = TqcHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8, 1.0, E, N, DROPPED)
            call = ctx.tqc_update
        else:
            hp = SacHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8)
            call = ctx.sac_update

        def fn():
            box["key"], box["count"] = call(pd, st["P"], st["pm"], st["pv"], qd, st["Q"], st["qm"], st["qv"], st["QT"], st["la"], st["am"],
                                            st["av"], batch, box["key"], box["count"], hp, met)

        ms = timed(fn, args.warmup, args.iters)
        assert torch.isfinite(met).all(), met
        row = {"what": kind + "_update", "critics": E, "batch": B, "ms": round(ms, 4), "updates_per_s": round(1000.0 / ms, 1)}
        print(json.dumps(row), flush=True)

    for E, B in configs:
        run("tqc", E, B)
    if not args.no_sac:
        for B in sorted({b for _, b in configs}):
            run("sac", 2, B)


if __name__ == "__main__":
    main()
