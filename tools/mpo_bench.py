"""Time one MPO update (rlx_mpo_update_f32) at the reference defaults (obs 48, act 12, hidden 256, 51 atoms, S = 20) for batch 256
and 4096, and acting (rlx_mpo_act_f32) at 4096 envs, on one MI355X.  Prints ms per call, updates / s, the FLOP model below and the
achieved TF/s.

    python tools/mpo_bench.py [--iters 50] [--warmup 10]

FLOP model (multiply-adds x 2, computed, not measured), R = 2B stacked rows, T = 3 S B target-critic rows:
  target critic   T (2 A H + 2 * 2 H^2 + 2 H NA) + R 2 Oc H          (the S-fold first layer is only its action part per sample)
  target policy   R 2 (Op H + 2 H^2 + 2 A H)
  online critic   3 B 2 ((Oc + A) H + 2 H^2 + H NA)                    (forward + two backward products)
  online policy   3 R 2 (Op H + 2 H^2 + 2 A H)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rl-x_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def flops(B, S=20, O=48, A=12, H=256, NA=51):
    R, T = 2 * B, 3 * S * B
    tc = T * (2 * A * H + 4 * H * H + 2 * H * NA) + R * 2 * O * H
    tp = R * 2 * (O * H + 2 * H * H + 2 * A * H)
    oc = 3 * B * 2 * ((O + A) * H + 2 * H * H + H * NA)
    op = 3 * R * 2 * (O * H + 2 * H * H + 2 * A * H)
    return tc + tp + oc + op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import mpo_twin as tw
    from rlx_amd.hip import Ctx, MpoHparams, mpo_desc
    from rlx_amd.hip import lib as L
    dev = torch.device("cuda:0")
    ctx = Ctx(0)
    O, A, H, NA, S = 48, 12, 256, 51, 20
    desc = mpo_desc(O, O, A, H, NA)
    h = tw.HP
    hp = MpoHparams()
    for k in ("gamma", "v_min", "v_max", "max_grad_norm", "epsilon_non_parametric", "epsilon_parametric_mu", "epsilon_parametric_sigma",
              "epsilon_penalty", "policy_init_scale", "policy_min_scale", "float_epsilon", "min_log_temperature", "min_log_alpha"):
        setattr(hp, k, float(h[k]))
    hp.adam_b1, hp.adam_b2, hp.adam_eps = 0.9, 0.999, 1e-8
    hp.action_sampling_number, hp.action_clipping, hp.action_rescaling = S, 1, 1
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    p, q = tw.make_params(1, O, O, A, H, NA)
    nets = [t(p), t(np.zeros_like(p)), t(np.zeros_like(p)), t(p), t(q), t(np.zeros_like(q)), t(np.zeros_like(q)), t(q),
            t(tw.init_duals(A, h)), t(np.zeros(2 * A + 2)), t(np.zeros(2 * A + 2))]
    rng = np.random.default_rng(0)
    results = []
    for B in (256, 4096):
        batch = (t(rng.standard_normal((B, O))), t(rng.standard_normal((B, O))), t(rng.uniform(-1, 1, (B, A))), t(rng.standard_normal(B)),
                 t(rng.random(B) < 0.1), t(np.zeros(B)), t(rng.integers(1, 5, B)))
        met = torch.zeros(17, device=dev)
        key = L.prng_key(0)
        step = 0
        for _ in range(args.warmup):
            step += 1
            key = ctx.mpo_update(desc, nets, batch, key, step, 3e-4, 1e-2, hp, met)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            step += 1
            key = ctx.mpo_update(desc, nets, batch, key, step, 3e-4, 1e-2, hp, met)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.iters
        f = flops(B, S, O, A, H, NA)
        assert torch.isfinite(met).all(), met
        results.append({"what": "update", "batch": B, "S": S, "ms": round(ms, 4), "updates_per_s": round(1000.0 / ms, 1),
                        "gflop_model": round(f / 1e9, 3), "tflops": round(f / (ms * 1e-3) / 1e12, 3)})
    N = 4096
    obs = t(rng.standard_normal((N, O)))
    act, proc = torch.empty(N, A, device=dev), torch.empty(N, A, device=dev)
    low, high = t(-np.ones(A)), t(np.ones(A))
    key = L.prng_key(1)
    for _ in range(args.warmup):
        key = ctx.mpo_act(desc, nets[0], obs, key, act, proc, hp, low, high)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        key = ctx.mpo_act(desc, nets[0], obs, key, act, proc, hp, low, high)
    e1.record()
    torch.cuda.synchronize()
    results.append({"what": "act", "nr_envs": N, "ms": round(e0.elapsed_time(e1) / args.iters, 4)})
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
