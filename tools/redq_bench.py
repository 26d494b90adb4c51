"""Time one REDQ update (rlx_redq_update_f32: G critic steps on G batches, then one policy step) at the reference's defaults --
ensemble 10, 2 in the target minimum, 20 critic steps, hidden 256 -- at obs 376, act 17, for batches of 256 and 4096 rows on one
MI355X, and -- same shapes, same process -- G + 1 SAC updates (rlx_sac_update_f32, two scalar critics) beside it: what the same
number of optimizer rounds costs on the fused twin-critic path.  Prints one JSON line per configuration: ms per call, calls / s and
(REDQ) critic steps / s.

    python tools/redq_bench.py [--iters 20] [--warmup 3] [--only E,M,G,B] [--no-sac]

Launches per call: trace the tool twice with different --iters for one configuration and divide the difference of the kernel
counts by the difference of the iteration counts (everything outside the timed loop cancels), e.g.
    rocprofv3 --kernel-trace --output-format csv -d out2 -- python tools/redq_bench.py --only 10,2,20,256 --no-sac --warmup 0 --iters 2
    rocprofv3 --kernel-trace --output-format csv -d out4 -- python tools/redq_bench.py --only 10,2,20,256 --no-sac --warmup 0 --iters 4
    (rows of out4/*kernel_trace.csv - rows of out2/*kernel_trace.csv) / 2"""
import argparse

from ens_bench import A, Bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="E,M,G,B: one REDQ configuration")
    ap.add_argument("--no-sac", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import RedqHparams
    bench = Bench(args)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(10, 2, 20, 256), (10, 2, 20, 4096)]
    for E, M, G, B in configs:
        st, b = bench.state(E), bench.batch(G, B)
        hp = RedqHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, M, G)
        bench.time_utd(bench.ctx.redq_update, bench.qdesc(), st, b, hp,
                       {"what": "redq_update", "critics": E, "in_target": M, "critic_steps": G, "batch": B})
    if not args.no_sac:
        for G, B in sorted({(c[2], c[3]) for c in configs}):
            bench.run_sac(G + 1, B)


if __name__ == "__main__":
    main()
