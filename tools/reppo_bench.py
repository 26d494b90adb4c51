#!/usr/bin/env python
"""`reppo.hip` iteration at the reference's default sizes (reppo/pytorch/default_config.py: 128 steps, 4 epochs x 128 minibatches,
policy / critic hidden 512, 151 bins, 16 KL samples) on the synthetic env: obs 48 / act 12 (assumed), 4096 envs (minibatch 4096
rows).  Reports ms per iteration split into rollout, targets and update, ms per minibatch update, env-steps/s, and the GFLOP of the
model below.  Not part of bench.py.

FLOP model (2 M N K per product; per row): policy forward P = 2 (O H + H H + H 2A); critic forward without / with the pred head
Q = 2 ((O + A) H + 3 H H + H NB), Qp = Q + 2 (H H + H (H + 1)).  Rollout step: P + P + Q (act, evaluate_next).  Critic step:
Qp + 2 Qp (forward, parameter + input gradients).  Policy step: 2 P (new + old policy) + Q + (2 Q on the action columns' input
gradient) + 2 P (policy backward)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))
import torch
from rlx_amd.runner.config_dict import ConfigDict
from rlx_amd.runner.default_config import get_config as runner_cfg
import rlx_amd.algorithms.reppo.hip, rlx_amd.environments.synthetic.random_obs  # noqa
from rlx_amd.algorithms.algorithm_manager import get_algorithm_config, get_algorithm_model_class
from rlx_amd.environments.environment_manager import get_environment_config, get_environment_create_train_and_eval_env

O, A, NE, H, NB = 48, 12, 4096, 512, 151


def flop_model(T, N, E, M):
    P = 2 * (O * H + H * H + H * 2 * A)
    Q = 2 * ((O + A) * H + 3 * H * H + H * NB)
    Qp = Q + 2 * (H * H + H * (H + 1))
    mb = T * N // M
    rollout = T * N * (2 * P + Q)
    critic = mb * 3 * Qp
    policy = mb * (2 * P + 3 * Q + 2 * P)
    return rollout, critic + policy, E * M * (critic + policy)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    config = ConfigDict()
    config.runner = runner_cfg("train")
    config.algorithm = get_algorithm_config("reppo.hip")
    config.environment = get_environment_config("synthetic.random_obs")
    config.environment.nr_envs, config.environment.obs_dim, config.environment.act_dim = NE, O, A
    config.algorithm.total_timesteps = NE * 128 * (iters + 1)
    env, _ = get_environment_create_train_and_eval_env("synthetic.random_obs")(config)
    m = get_algorithm_model_class("reppo.hip")(config, env, env, "/tmp/reppo_bench", None)
    m._alloc()
    state, _ = env.reset()
    state = state.clone()
    T, E, M = m.nr_steps, m.nr_epochs, m.nr_minibatches
    rows = []
    for it in range(iters + 1):            # the first iteration is a warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            state = m.rollout_step(state, t)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m.ctx.reppo_td_lambda(m.b_soft, m.b_nv, m.b_term, m.b_trunc, m.hp.gamma, m.hp.gae_lambda, m.b_targets)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        m.optimize()                       # targets again + snapshot + the whole update + the one host read
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it:
            rows.append((t1 - t0, t2 - t1, t3 - t2))
    ro, tg, up = (sum(r[i] for r in rows) / len(rows) * 1e3 for i in range(3))
    f_ro, f_mb, f_up = flop_model(T, NE, E, M)
    res = dict(ms_per_iteration=ro + tg + up, ms_rollout=ro, ms_targets=tg, ms_update=up, ms_per_minibatch=up / (E * M),
               env_steps_per_s=T * NE / ((ro + tg + up) / 1e3), gflop_rollout=f_ro / 1e9, gflop_per_minibatch=f_mb / 1e9,
               tflops_rollout=f_ro / (ro / 1e3) / 1e12, tflops_update=f_up / (up / 1e3) / 1e12)
    print({k: round(v, 3) for k, v in res.items()})


if __name__ == "__main__":
    main()
