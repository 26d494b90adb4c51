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

from ens_bench import A, Bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="E,H,dropped,G,B: one AQE configuration")
    ap.add_argument("--no-sac", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import AqeHparams
    bench = Bench(args)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(10, 2, 4, 5, 256), (10, 2, 4, 5, 4096)]
    for E, H, dropped, G, B in configs:
        st, b = bench.state(E, H), bench.batch(G, B)
        hp = AqeHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, H, dropped, G)
        bench.time_utd(bench.ctx.aqe_update, bench.qdesc(H), st, b, hp,
                       {"what": "aqe_update", "critics": E, "heads": H, "dropped": dropped, "critic_steps": G, "batch": B})
    if not args.no_sac:
        for G, B in sorted({(c[3], c[4]) for c in configs}):
            bench.run_sac(G + 1, B)


if __name__ == "__main__":
    main()
