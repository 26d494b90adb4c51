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

from ens_bench import A, Bench

N, DROPPED = 25, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="", help="E,B: one TQC configuration")
    ap.add_argument("--no-sac", action="store_true")
    args = ap.parse_args()
    from rlx_amd.hip import SacHparams, TqcHparams
    bench = Bench(args)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(2, 256), (5, 256), (2, 4096), (5, 4096)]

    def run(kind, E, B):
        out_dim = N if kind == "tqc" else 1
        st, b = bench.state(E, out_dim), tuple(x[0] for x in bench.batch(1, B))
        if kind == "tqc":
            hp = TqcHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8, 1.0, E, N, DROPPED)
            call = bench.ctx.tqc_update
        else:
            hp = SacHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8)
            call = bench.ctx.sac_update
        nets = bench.nets(bench.qdesc(out_dim), st)
        ms = bench.time_step(lambda key, count, met: call(*nets, b, key, count, hp, met), 1)
        row = {"what": kind + "_update", "critics": E, "batch": B, "ms": round(ms, 4), "updates_per_s": round(1000.0 / ms, 1)}
        print(json.dumps(row), flush=True)

    for E, B in configs:
        run("tqc", E, B)
    if not args.no_sac:
        for B in sorted({b for _, b in configs}):
            run("sac", 2, B)


if __name__ == "__main__":
    main()
