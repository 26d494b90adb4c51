"""Time one whole FastMPO update (rlx_fastmpo_update_f32: P 2 rounds of G 4 critic steps and one policy + dual step) at the reference
defaults -- obs 48, act 12, B 8192, K 4, 101 atoms, two critics, fastsac network kinds (policy 512-256-128, critics 768-384-192) --
beside one MPO update (rlx_mpo_update_f32, tools/mpo_bench.py's: hidden 256, 51 atoms, S 20) at the same batch, on one MI355X, with
tools/ens_bench.py's event timer.

    python tools/fastmpo_bench.py [--iters 20] [--warmup 5] [--only fastmpo|mpo]

Launch counts: `--launches DIR_A DIR_B` reads two kernel traces of this tool (rocprofv3 --kernel-trace --output-format csv -d DIR --
python tools/fastmpo_bench.py --only fastmpo --warmup 0 --iters 1, and the same with --iters 3) and prints (rows of B - rows of A) / 2,
the kernel launches of one call: everything outside the timed loop cancels.

FLOP model of the FastMPO line (multiply-adds x 2, computed, not measured): per critic step the E target critics on K B rows (their
first layer's observation part on B rows) and the E online critics forward + two backward products on B rows; per round the same
target pass on K 2B rows and the policy forward + two backward products on 2B rows; the target policy on B / 2B rows."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rl-x_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

O, A, B = 48, 12, 8192


def _mlp(d, hidden, out):
    f = 0
    for h in hidden:
        f, d = f + d * h, h
    return f + d * out


def flops(P, G, K, E, NA, ph, ch):
    pol, cri = _mlp(O, ph, 2 * A), _mlp(O + A, ch, NA)
    cri_samples = cri - O * ch[0]                         # per sampled action: everything but the observation part of layer 1
    target = lambda M: E * (K * M * cri_samples + M * O * ch[0])
    critic_step = target(B) + B * pol + 3 * E * B * cri
    policy_step = target(2 * B) + 2 * B * pol + 3 * 2 * B * pol
    return 2 * P * (G * critic_step + policy_step)


def fastmpo_line(args, ctx, dev):
    import fastmpo_cases as fc
    import fastmpo_twin as tw
    from ens_bench import timed
    h = dict(tw.HP)
    P, G, K, E, NA = h["nr_policy_updates_per_step"], h["nr_critic_updates_per_policy_update"], h["action_sampling_number"], 2, 101
    c = fc.Case(1, "fastsac", E=E, O=O, A=A, NA=NA, B=B, K=K, P=P, G=G, policy_hidden=tw.POLICY_WIDTHS["fastsac"],
                critic_hidden=tw.CRITIC_WIDTHS["fastsac"])
    nets = tuple(fc._t(c.st[k], dev) for k in fc.STATE_KEYS)
    batch = tuple(fc._t(x, dev) for x in c.batches)
    hp, met, box = fc.hparams(c.h), torch.zeros(len(tw.METRICS), device=dev), [(0, 0, 0)]

    def fn():
        box[0] = ctx.fastmpo_update(c.desc, nets, batch, np.array([0, box[0][0]], np.uint32), box[0], *c.lrs, hp, met)

    ms = timed(fn, args.warmup, args.iters)
    assert torch.isfinite(met).all(), met
    f = flops(P, G, K, E, NA, tw.POLICY_WIDTHS["fastsac"], tw.CRITIC_WIDTHS["fastsac"])
    return {"what": "fastmpo_update", "batch": B, "K": K, "critics": E, "atoms": NA, "P": P, "G": G, "ms": round(ms, 3),
            "ms_per_critic_step": round(ms / (P * G), 3), "updates_per_s": round(1000.0 / ms, 2), "gflop_model": round(f / 1e9, 2),
            "tflops": round(f / (ms * 1e-3) / 1e12, 2)}


def mpo_line(args, ctx, dev):
    import mpo_cases
    import mpo_twin as tw
    from ens_bench import timed
    from mpo_bench import flops as mpo_flops
    from rlx_amd.hip import mpo_desc
    from rlx_amd.hip import lib as L
    H, NA, S = 256, 51, 20
    h = dict(tw.HP)
    hp = mpo_cases._hp(h)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    p, q = tw.make_params(1, O, O, A, H, NA)
    nets = [t(p), t(np.zeros_like(p)), t(np.zeros_like(p)), t(p), t(q), t(np.zeros_like(q)), t(np.zeros_like(q)), t(q),
            t(tw.init_duals(A, h)), t(np.zeros(2 * A + 2)), t(np.zeros(2 * A + 2))]
    rng = np.random.default_rng(0)
    batch = (t(rng.standard_normal((B, O))), t(rng.standard_normal((B, O))), t(rng.uniform(-1, 1, (B, A))), t(rng.standard_normal(B)),
             t(rng.random(B) < 0.1), t(np.zeros(B)), t(rng.integers(1, 5, B)))
    met, box = torch.zeros(17, device=dev), [L.prng_key(0), 0]

    def fn():
        box[1] += 1
        box[0] = ctx.mpo_update(mpo_desc(O, O, A, H, NA), nets, batch, box[0], box[1], 3e-4, 1e-2, hp, met)

    ms = timed(fn, args.warmup, args.iters)
    assert torch.isfinite(met).all(), met
    f = mpo_flops(B, S, O, A, H, NA)
    return {"what": "mpo_update", "batch": B, "S": S, "atoms": NA, "hidden": H, "ms": round(ms, 3), "updates_per_s": round(1000.0 / ms, 2),
            "gflop_model": round(f / 1e9, 2), "tflops": round(f / (ms * 1e-3) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("fastmpo", "mpo"))
    ap.add_argument("--launches", nargs=2, metavar="DIR", help="two trace directories (--iters 1 and --iters 3): print launches per call")
    args = ap.parse_args()
    if args.launches:
        import csv
        import glob
        rows = [sum(sum(1 for _ in csv.reader(open(f))) - 1 for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True)) for d in args.launches]
        print(json.dumps({"what": "launches_per_call", "rows": rows, "launches": (rows[1] - rows[0]) / 2}), flush=True)
        return
    from rlx_amd.hip import Ctx
    dev = torch.device("cuda:0")
    ctx = Ctx(0)
    for name, fn in (("fastmpo", fastmpo_line), ("mpo", mpo_line)):
        if args.only in (None, name):
            print(json.dumps(fn(args, ctx, dev)), flush=True)


if __name__ == "__main__":
    main()
