"""Time one TD3 update (rlx_td3_update_f32: the critic step and the policy step with both Polyak updates) and one DDPG update (one
critic, the joint step) at the reference's defaults -- batch 256, hidden 256-256 -- at tools/ens_bench.py's shapes (obs 376, act 17)
on one MI355X, and -- same shapes, same process -- one SAC update (rlx_sac_update_f32, two scalar critics) beside them.  Prints one
JSON line per configuration: ms per call and calls / s.

    python tools/td3_bench.py [--iters 200] [--warmup 20] [--batch 256] [--only td3|td3_critic|ddpg|sac]

Launches per call: trace the tool twice with different --iters for one configuration and divide the difference of the kernel
counts by the difference of the iteration counts (everything outside the timed loop cancels), e.g.
    rocprofv3 --kernel-trace --output-format csv -d out2 -- python tools/td3_bench.py --only td3 --warmup 0 --iters 2
    rocprofv3 --kernel-trace --output-format csv -d out4 -- python tools/td3_bench.py --only td3 --warmup 0 --iters 4
    (rows of out4/*kernel_trace.csv - rows of out2/*kernel_trace.csv) / 2"""
import argparse
import json

import numpy as np
import torch

from ens_bench import A, O, W, Bench, lecun


def run_td3(bench, what, B, nr_critics, joint, policy_step):
    from rlx_amd.hip import ACT_RELU, Td3Hparams, mlp_desc
    pd = mlp_desc(O, [W, W], A, ACT_RELU, False, False)
    qd = bench.qdesc()
    P = bench.t(lecun(bench.rng, O, [W, W], A))
    Q = bench.t(np.concatenate([lecun(bench.rng, O + A, [W, W], 1) for _ in range(nr_critics)]))
    z = torch.zeros_like
    b = tuple(x[0] for x in bench.batch(1, B))
    hp = Td3Hparams(0.99, 0.005, 0.0 if joint else 0.2, 0.5, 3e-4, 3e-4, 0.9, 0.999, 1e-8, nr_critics, int(joint), int(policy_step))
    nets = (pd, P, z(P), z(P), P.clone(), qd, Q, z(Q), z(Q), Q.clone())
    ms = bench.time_step(lambda key, q, pi, met: bench.ctx.td3_update(*nets, b, key, q, pi, hp, met), 2)
    print(json.dumps({"what": what, "critics": nr_critics, "policy_step": int(policy_step), "batch": B, "ms": round(ms, 4),
                      "calls_per_s": round(1000.0 / ms, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default="", help="td3, td3_critic, ddpg or sac: one configuration")
    args = ap.parse_args()
    bench = Bench(args)
    for what, cfg in (("td3", (2, False, True)), ("td3_critic", (2, False, False)), ("ddpg", (1, True, True))):
        if args.only in ("", what):
            run_td3(bench, what + "_update", args.batch, *cfg)
    if args.only in ("", "sac"):
        bench.run_sac(1, args.batch)


if __name__ == "__main__":
    main()
