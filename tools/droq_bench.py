"""Time one DroQ update (rlx_droq_update_f32: G critic steps on G batches, then one policy step) at the reference's defaults -- two
Dropout(0.01) -> LayerNorm -> ReLU critics, both in the target minimum, 20 critic steps, hidden 256 -- at obs 376, act 17, for
batches of 256 and 4096 rows on one MI355X, and -- same shapes, same process -- one REDQ update (rlx_redq_update_f32, plain ReLU
critics) at E 2 / M 2 / G 20, which shows what LayerNorm and dropout cost, and one at REDQ's own defaults E 10.  Prints one JSON line
per configuration: ms per call, calls / s and critic steps / s.

    python tools/droq_bench.py [--iters 20] [--warmup 3] [--only E,M,G,B] [--rate 0.01] [--no-redq]

Launches per call: trace the tool twice with different --iters for one configuration and divide the difference of the kernel
counts by the difference of the iteration counts (everything outside the timed loop cancels), e.g.
    rocprofv3 --kernel-trace --output-format csv -d out1 -- python tools/droq_bench.py --only 2,2,20,256 --no-redq --warmup 0 --iters 1
    rocprofv3 --kernel-trace --output-format csv -d out3 -- python tools/droq_bench.py --only 2,2,20,256 --no-redq --warmup 0 --iters 3
    (rows of out3/*kernel_trace.csv - rows of out1/*kernel_trace.csv) / 2; the k_drop_ln_relu rows of the same trace give its time"""
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

O, A, H = 376, 17, 256


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
    ap.add_argument("--only", default="", help="E,M,G,B: one DroQ configuration")
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--no-redq", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import ACT_RELU, Ctx, DroqHparams, RedqHparams, mlp_desc
    from rlx_amd.hip import lib as L
    dev = torch.device("cuda:0")
    ctx = Ctx(0)
    rng = np.random.default_rng(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    pd = mlp_desc(O, [H, H], 2 * A, ACT_RELU, False, False)
    qd = mlp_desc(O + A, [H, H], 1, ACT_RELU, False, False)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(2, 2, 20, 256), (2, 2, 20, 4096)]

    def with_layer_norm(flat):                                 # LayerNorm scale 1, bias 0 after every hidden bias (csrc/droq.hip's layout)
        parts, off, d = [], 0, O + A
        for h in (H, H):
            n = d * h + h
            parts += [flat[off:off + n], np.ones(h, np.float32), np.zeros(h, np.float32)]
            off, d = off + n, h
        return np.concatenate(parts + [flat[off:]])

    def state(E, layer_norm=False):
        pp = lecun(rng, O, [H, H], 2 * A)
        pp[-(H * 2 * A + 2 * A):] *= 0.1                       # std ~ 1: the tanh rarely saturates
        P = t(pp)
        nets = [lecun(rng, O + A, [H, H], 1) for _ in range(E)]
        Q = t(np.concatenate([with_layer_norm(x) if layer_norm else x for x in nets]))
        return dict(P=P, pm=torch.zeros_like(P), pv=torch.zeros_like(P), Q=Q, qm=torch.zeros_like(Q), qv=torch.zeros_like(Q), QT=Q.clone(),
                    la=torch.zeros(1, device=dev), am=torch.zeros(1, device=dev), av=torch.zeros(1, device=dev))

    def batch(G, B):
        return (t(rng.standard_normal((G, B, O))), t(rng.standard_normal((G, B, O))), t(np.tanh(rng.standard_normal((G, B, A)))),
                t(rng.standard_normal((G, B))), t(rng.random((G, B)) < 0.1))

    def run(what, E, M, G, B):
        droq = what == "droq_update"
        st, bt, met = state(E, droq), batch(G, B), torch.zeros(10, device=dev)
        hp = (DroqHparams if droq else RedqHparams)(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, M, G)
        if droq:
            hp.dropout_rate = args.rate
        update = ctx.droq_update if droq else ctx.redq_update
        box = dict(key=L.prng_key(0), q=0, pi=0)

        def fn():
            box["key"], box["q"], box["pi"] = update(pd, st["P"], st["pm"], st["pv"], qd, st["Q"], st["qm"], st["qv"], st["QT"], st["la"],
                                                     st["am"], st["av"], bt, box["key"], box["q"], box["pi"], hp, met)

        ms = timed(fn, args.warmup, args.iters)
        assert torch.isfinite(met).all(), met
        row = {"what": what, "critics": E, "in_target": M, "critic_steps": G, "batch": B, "ms": round(ms, 3),
               "calls_per_s": round(1000.0 / ms, 2), "critic_steps_per_s": round(1000.0 * G / ms, 1)}
        if droq:
            row["dropout_rate"] = args.rate
        print(json.dumps(row), flush=True)

    for E, M, G, B in configs:
        run("droq_update", E, M, G, B)
        if not args.no_redq:
            run("redq_update", E, M, G, B)
            run("redq_update", 10, 2, G, B)


if __name__ == "__main__":
    main()
