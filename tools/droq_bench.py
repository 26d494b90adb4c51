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

import numpy as np

from ens_bench import A, O, W, Bench


def with_layer_norm(flat):                                     # LayerNorm scale 1, bias 0 after every hidden bias (csrc/droq.hip's layout)
    parts, off, d = [], 0, O + A
    for h in (W, W):
        n = d * h + h
        parts += [flat[off:off + n], np.ones(h, np.float32), np.zeros(h, np.float32)]
        off, d = off + n, h
    return np.concatenate(parts + [flat[off:]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="E,M,G,B: one DroQ configuration")
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--no-redq", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import DroqHparams, RedqHparams
    bench = Bench(args)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(2, 2, 20, 256), (2, 2, 20, 4096)]

    def run(what, E, M, G, B):
        droq = what == "droq_update"
        st, b = bench.state(E, 1, with_layer_norm if droq else None), bench.batch(G, B)
        hp = (DroqHparams if droq else RedqHparams)(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, M, G)
        if droq:
            hp.dropout_rate = args.rate
        bench.time_utd(bench.ctx.droq_update if droq else bench.ctx.redq_update, bench.qdesc(), st, b, hp,
                       {"what": what, "critics": E, "in_target": M, "critic_steps": G, "batch": B},
                       **({"dropout_rate": args.rate} if droq else {}))

    for E, M, G, B in configs:
        run("droq_update", E, M, G, B)
        if not args.no_redq:
            run("redq_update", E, M, G, B)
            run("redq_update", 10, 2, G, B)


if __name__ == "__main__":
    main()
