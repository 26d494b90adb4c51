"""One PPO-DTRL update (rlx_dtrl_update_f32) beside one PPO update (rlx_ppo_update_f32) at the same shape, on tools/ens_bench.py's
event timer: full-jit nets (512 LayerNorm ELU, 256, 128), one rollout of T x N rows, E epochs of minibatches of mb rows.  Prints one
JSON line.  The DTRL call computes the rollout means itself (old_means = NULL), as the plugin runs it.

    python tools/dtrl_bench.py [--obs 48] [--act 12] [--envs 4096] [--steps 32] [--mb 32768] [--epochs 2] [--warmup 2] [--iters 5]
"""
import argparse
import json

import numpy as np
import torch

from ens_bench import timed
from rlx_amd.algorithms.ppo.hip.ppo import init_flat_params
from rlx_amd.hip import ACT_ELU, Ctx, DtrlHparams, PpoHparams, mlp_desc
from rlx_amd.hip import lib as L


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("obs", 48), ("act", 12), ("envs", 4096), ("steps", 32), ("mb", 32768), ("epochs", 2), ("warmup", 2), ("iters", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx, rng = torch.device("cuda:0"), Ctx(0), np.random.default_rng(0)
    hidden, T, N = [512, 256, 128], a.steps, a.envs
    pd, cd = mlp_desc(a.obs, hidden, a.act, ACT_ELU, True, True), mlp_desc(a.obs, hidden, 1, ACT_ELU, True, False)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    p0, c0 = t(init_flat_params(rng, a.obs, hidden, a.act, True, True, 0.01, 1.0)), t(init_flat_params(rng, a.obs, hidden, 1, True, False, 1.0, 1.0))
    states, actions = t(rng.normal(0, 1, (T, N, a.obs))), t(rng.normal(0, 1, (T, N, a.act)))
    # log-probs of the actions under the initial policy (mean ~ 0, std 1) plus a little noise: ratios near 1, as after a rollout
    logp = (-0.5 * (actions ** 2).sum(-1) - 0.9189385 * a.act + t(0.05 * rng.normal(0, 1, (T, N)))).contiguous()
    ret, adv = t(rng.normal(0, 1, (T, N))), t(rng.normal(0, 1, (T, N)))
    n_upd = a.epochs * (T * N // a.mb)
    lrs = np.full(n_upd, 4e-4, np.float32)
    key = L.prng_key(1)
    php = PpoHparams(0.1, 0.0, 1.0, 5.0, 0.9, 0.999, 1e-8)
    dhp = DtrlHparams(0.1, 0.0, 1.0, 5.0, 0.9, 0.999, 1e-8, 0.03, 0.001, 0.1, 2e9, None)
    out = {"shape": {"obs": a.obs, "act": a.act, "T": T, "N": N, "minibatch": a.mb, "epochs": a.epochs, "steps_per_update": n_upd}}
    for name in ("ppo", "dtrl"):
        nets = [x.clone() for x in (p0, torch.zeros_like(p0), torch.zeros_like(p0), c0, torch.zeros_like(c0), torch.zeros_like(c0))]
        met = torch.zeros(n_upd, 10 if name == "ppo" else 14, device=dev)

        def one():
            if name == "ppo":
                ctx.ppo_update(pd, *nets[:3], cd, *nets[3:], states, actions, logp, ret, adv, a.epochs, a.mb, key, 0, lrs, php, met)
            else:
                ctx.dtrl_update(pd, *nets[:3], cd, *nets[3:], states, actions, None, logp, ret, adv, a.epochs, a.mb, key, 0, lrs,
                                float(T * N), dhp, met)
        ms = timed(one, a.warmup, a.iters)
        out[name + "_metrics_finite"] = bool(torch.isfinite(met).all())
        out[name + "_update_ms"] = round(ms, 3)
        out[name + "_step_us"] = round(1e3 * ms / n_upd, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
