"""Time CrossQ's two update calls (rlx_crossq_critic_update_f32, rlx_crossq_policy_update_f32) at obs 376, act 17, policy hidden 256,
E 2 critics of hidden width 1024 and 2048 (the reference's default), for batches of 256 and 4096 rows on one MI355X, and -- same
process, same batch -- one SAC update (rlx_sac_update_f32, two 256-wide critics) as context.  Prints one JSON line per
configuration: ms per critic update and per policy update.

    python tools/crossq_bench.py [--iters 20] [--warmup 3] [--only WIDTH,B] [--what critic|policy|both] [--no-sac]

Launch counts: `--launches DIR_A DIR_B` reads two kernel traces of this tool (rocprofv3 --kernel-trace --output-format csv -d DIR --
python tools/crossq_bench.py --only WIDTH,B --what critic --no-sac --warmup 0 --iters N) taken at --iters 1 and --iters 3 and prints
(rows of B - rows of A) / 2, the kernel launches of one call: everything outside the timed loop cancels."""
import argparse
import json

import numpy as np
import torch



def with_brn(flat, in_dim, hidden, out_dim):                   # scale 1, bias 0 in front of every Dense (csrc/crossq.hip's layout)
    parts, off, d = [], 0, in_dim
    for h in list(hidden) + [out_dim]:
        n = d * h + h
        parts += [np.ones(d, np.float32), np.zeros(d, np.float32), flat[off:off + n]]
        off, d = off + n, h
    return np.concatenate(parts)


def fresh_stats(in_dim, hidden):
    return np.concatenate([np.concatenate([np.zeros(d, np.float32), np.ones(d, np.float32)]) for d in [in_dim] + list(hidden)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="WIDTH,B: one configuration")
    ap.add_argument("--no-sac", action="store_true")
    ap.add_argument("--what", default="both", choices=("critic", "policy", "both"))
    ap.add_argument("--launches", nargs=2, metavar="DIR", help="two trace directories (--iters 1 and --iters 3): print launches per call")
    args = ap.parse_args()
    if args.launches:
        import csv
        import glob
        rows = [sum(sum(1 for _ in csv.reader(open(f))) - 1 for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True)) for d in args.launches]
        print(json.dumps({"what": "launches_per_call", "rows": rows, "launches": (rows[1] - rows[0]) / 2}), flush=True)
        return
    from ens_bench import A, O, W, Bench, lecun
    from rlx_amd.hip import ACT_RELU, mlp_desc
    from rlx_amd.hip import lib as L
    bench = Bench(args)
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else [(1024, 256), (2048, 256), (1024, 4096), (2048, 4096)]
    E = 2
    for width, B in configs:
        qh = [width, width]
        qd = mlp_desc(O + A, qh, 1, ACT_RELU, False, False)
        pp = lecun(bench.rng, O, [W, W], 2 * A)
        pp[-(W * 2 * A + 2 * A):] *= 0.1
        P = bench.t(with_brn(pp, O, [W, W], 2 * A))
        Q = bench.t(np.concatenate([with_brn(lecun(bench.rng, O + A, qh, 1), O + A, qh, 1) for _ in range(E)]))
        ps, qs = bench.t(fresh_stats(O, [W, W])), bench.t(np.concatenate([fresh_stats(O + A, qh)] * E))
        pm, pv, qm, qv = (torch.zeros_like(x) for x in (P, P, Q, Q))
        la, am, av = (torch.zeros(1, device=bench.dev) for _ in range(3))
        b = tuple(x[0] for x in bench.batch(1, B))
        hp = L.CrossqHparams(0.99, -float(A), -20.0, 2.0, 1e-3, 1e-3, 1e-3, 0.5, 0.5, 0.9, 0.999, 1e-8, 0.99, 1e-3, 3.0, 5.0, 100000, E)
        ctx = bench.ctx
        row = {"what": "crossq", "critics": E, "critic_width": width, "batch": B}
        if args.what != "policy":
            row["ms_critic_update"] = round(bench.time_step(
                lambda key, n, met: ctx.crossq_critic_update(bench.pd, P, ps, qd, Q, qm, qv, qs, la, b, key, n, hp, met), 1), 3)
        if args.what != "critic":
            row["ms_policy_update"] = round(bench.time_step(
                lambda key, n, met: ctx.crossq_policy_update(bench.pd, P, pm, pv, ps, qd, Q, qs, la, am, av, b[0], key, n, hp, met), 1), 3)
        print(json.dumps(row), flush=True)
        if not args.no_sac and width == configs[0][0]:
            bench.run_sac(1, B)


if __name__ == "__main__":
    main()
