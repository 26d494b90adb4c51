#!/usr/bin/env python
"""`fasttd3.hip` vector step at the reference's default update sizes (fasttd3/pytorch/default_config.py: batch 32768, 1 policy x 2
critic updates per step, nr_atoms 101, critics 1024-512-256) on the synthetic env: obs 48 / act 12 (assumed), 4096 envs.  The ring
holds 64 steps per env instead of the default 10240 (18.6 GB less memory; the cost of sampling does not depend on the length of the ring).  Reports ms per
vector step, critic updates/s, the GFLOP per step of the model below and the fraction of the split-fp32 engine peak.

FLOP model (2 M N K per product; per row): one critic forward 1.49 MFLOP, the policy forward 0.38; a critic step = policy forward
+ 2 target + 2 online forwards + 2 backwards without the first layer's input gradient; a policy step = policy forward + 2 critic
forwards + 2 critic backwards without parameter gradients (the first layer's input gradient on the action columns only) + the
policy's backward."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))
import torch
from rlx_amd.runner.config_dict import ConfigDict
from rlx_amd.runner.default_config import get_config as runner_cfg
import rlx_amd.algorithms.fasttd3.hip, rlx_amd.environments.synthetic.random_obs  # noqa
from rlx_amd.algorithms.algorithm_manager import get_algorithm_config, get_algorithm_model_class
from rlx_amd.environments.environment_manager import get_environment_config, get_environment_create_train_and_eval_env

PEAK_TF = 833.3      # split-fp32 ("fp16 x 3") engine peak, DESIGN.md 4.1
O, A, NA, NE = 48, 12, 101, 4096


def layers(i, hidden, o):
    dims = [i] + list(hidden) + [o]
    return list(zip(dims[:-1], dims[1:]))


def flop_model(B, nc, npol):
    Lq, Lp = layers(O + A, (1024, 512, 256), NA), layers(O, (512, 256, 128), A)
    fwd = lambda L: sum(2 * k * n for k, n in L)
    q_f, p_f = fwd(Lq), fwd(Lp)
    q_bwd_params = 2 * q_f - 2 * Lq[0][0] * Lq[0][1]                        # dW of every layer + dX of every layer but the first
    q_bwd_dx = q_f - 2 * Lq[0][0] * Lq[0][1] + 2 * A * Lq[0][1]              # dX only; the first layer's on the A action columns
    p_bwd = 2 * p_f - 2 * Lp[0][0] * Lp[0][1]
    critic_step = p_f + 4 * q_f + 2 * q_bwd_params
    policy_step = p_f + 2 * q_f + 2 * q_bwd_dx + p_bwd
    return B * (nc * critic_step + npol * policy_step), q_f, p_f


config = ConfigDict()
config.runner = runner_cfg("train")
config.algorithm = get_algorithm_config("fasttd3.hip")
config.environment = get_environment_config("synthetic.random_obs")
config.environment.nr_envs, config.environment.obs_dim, config.environment.act_dim = NE, O, A
config.algorithm.buffer_size_per_env = 64
env, _ = get_environment_create_train_and_eval_env("synthetic.random_obs")(config)
m = get_algorithm_model_class("fasttd3.hip")(config, env, env, "/tmp/x", None)
m._alloc()
m.redraw_noise_scales()
state, _ = env.reset(); state = state.clone()
nc, npol, B = m.nr_critic_updates * m.nr_policy_updates, m.nr_policy_updates, m.batch_size


def vector_step(state, k):
    action, processed = m.act_pair(state)
    ns, r, term, trunc, info = env.step(processed)
    done = (term | trunc).float()
    m.replay_add(state, ns, action, r, done, trunc.float())
    m.redraw_noise_scales(done)
    m.optimize(k)
    return ns.clone()


for k in range(4): state = vector_step(state, k)
flops, q_f, p_f = flop_model(B, nc, npol)
K = 20
for rep in range(2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for k in range(K): state = vector_step(state, k)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    ms = 1e3 * dt / K
    print(f"FastTD3 (batch {B}, ring {m.capacity} per env): {ms:.2f} ms per vector step (host {1e3 * t_host / K:.2f}), {nc * K / dt:.0f} critic updates/s, "
          f"{flops / 1e9:.0f} GFLOP per step (critic fwd {q_f / 1e6:.2f}, policy fwd {p_f / 1e6:.2f} MFLOP/row), "
          f"{flops / (ms * 1e-3) / 1e12:.1f} TF/s = {flops / (ms * 1e-3) / 1e12 / PEAK_TF:.3f} of the {PEAK_TF:.0f} TF engine peak")
print("finite:", bool(torch.isfinite(m.metrics_c).all() and torch.isfinite(m.metrics_p).all()), m.metrics_c.cpu().tolist(),
      m.metrics_p.cpu().tolist())
