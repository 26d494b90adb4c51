"""`fastmpo.hip`: the FastMPO training loop of rl_x/algorithms/fastmpo/flax_full_jit/fastmpo.py:198-714 around the library's update
(rl-x_amd/csrc/fastmpo.hip).

`learning_starts` vector steps fill the ring with the acting policy's samples (:227-267; they do not count as env steps).  Then per
learning iteration (:277-631): act on the normalised observation with the TARGET policy (the online one with
collect_data_with_online_policy), env.step, ring add -- the ring's next state is the observation the episode ended on where it
ended (:247 env_state.actual_next_observation: the env's `final_observation`, not the auto-reset one); ONE sample of all P G
batches (:494-548: rlx_sac_replay_draw_i32 + rlx_fastsac_replay_sample_f32); the normaliser merged ONCE with the concatenated [states_all; next_states_all] rows and applied to
both (:550-567: one rlx_obs_norm_update_f32 call on 2 P G B rows); ONE rlx_fastmpo_update_f32 call for the P rounds of G critic
steps and one policy + dual step (:572-627).  Learning rates follow the optimisers' own step counts when annealed (:126-146).
Evaluation (:671-702) is the loop's `evaluate` with the online policy's mean.

Where the existing sampler differs from fastmpo.py:497-503 and this file makes up for it: with n_steps == 1 the ring's sampler
returns the stored truncations; the reference counts a FULL ring's newest row as truncated unless it is done, for every n_steps.
`patch_newest_truncation` applies that (it never changes a loss: a row that is not done bootstraps whatever its truncation flag).

What differs from the reference, on purpose: random numbers (the library's counter RNG for the replay indices -- one key for both
index vectors, as sac.hip's fully jitted flavour draws them -- and the acting noise; the update's per-row keys are addressed as
the reference addresses them), parameters initialised from numpy with the reference's schemes (flax Dense: lecun-normal weights,
zero bias; LayerNorm 1 / 0; the heads as policy.py / critic.py give them), single GPU, nr_parallel_seeds == 1 (refused otherwise,
as the reference refuses it)."""
import json
import logging
import os
import time

import numpy as np

from rlx_amd.algorithms.fast_offpolicy import FastOffPolicyLoop
from rlx_amd.algorithms.fastmpo.hip.general_properties import GeneralProperties
from rlx_amd.environments.data_interface_type import DataInterfaceType
from rlx_amd.plugin import MetricSink, adopt_checkpoint_config

rlx_logger = logging.getLogger("rl_x")

KINDS = ("fastsac", "fasttd3", "mpo")
RESCALING = ("none", "normal", "fastsac")
CRITIC_METRICS = ("loss/q_loss", "q/q_mean", "q/q_max", "q/q_min", "lr/critic_learning_rate", "gradients/critic_grad_norm")
POLICY_METRICS = ("loss/actor_loss", "loss/loss_pg_mean", "loss/loss_pg_std", "loss/loss_kl_mean", "loss/loss_kl_std", "loss/dual_loss",
                  "loss/loss_alpha_mean", "loss/loss_alpha_std", "loss/loss_eta", "dual/eta", "dual/penalty_temperature", "dual/alpha_mean",
                  "dual/alpha_std", "kl/mean_kl_mean", "kl/mean_kl_std", "q/improvement_q_mean", "policy/std_min_mean",
                  "policy/std_max_mean", "lr/policy_learning_rate", "lr/dual_variables_learning_rate", "gradients/policy_grad_norm",
                  "gradients/dual_variables_grad_norm")
METRIC_NAMES = CRITIC_METRICS + POLICY_METRICS        # fastmpo.py:372-377, :595-596, :461-480, :624-627: rlx_fastmpo_update_f32's order
TRUNC_NORMAL_STD = 0.87962566103423978               # std of a unit normal truncated at +-2 (jax.nn.initializers.variance_scaling)


def _truncated_normal(rng, shape, std):
    x = rng.standard_normal(shape)
    while True:
        out = np.abs(x) > 2.0
        if not out.any():
            return x * (std / TRUNC_NORMAL_STD)
        x[out] = rng.standard_normal(int(out.sum()))


def patch_newest_truncation(xp, idx_t, dones, truncations, last):
    """fastmpo.py:497-503 on sampled rows: a row drawn from the ring's newest slot `last` counts as truncated unless it is done.
    xp: torch or numpy (both have `where` and `ones_like`)"""
    return xp.where((idx_t == last) & (dones <= 0.0), xp.ones_like(truncations), truncations)


def init_params(rng, kind, in_dim, hidden, heads):
    """flat layout of include/rlx_hip.h (rlx_fastmpo_desc).  Hidden Dense layers: flax's default lecun_normal (fastsac, fasttd3) or
    uniform_scaling(0.333) (mpo: +-sqrt(3 / fan_in) 0.333), zero bias, LayerNorm 1 / 0 where the layer has one.  heads: a list of
    (width, scheme, value) column groups of the head, side by side: "zeros", "normal" (stddev value), "lecun", or "variance"
    (variance_scaling(value, fan_in, truncated_normal))."""
    parts, d = [], in_dim
    for li, h in enumerate(hidden):
        if kind == "mpo":
            bound = np.sqrt(3.0 / d) * 0.333
            parts += [rng.uniform(-bound, bound, (d, h)), np.zeros(h)]
        else:
            parts += [_truncated_normal(rng, (d, h), np.sqrt(1.0 / d)), np.zeros(h)]
        if kind == "fastsac" or (kind == "mpo" and li == 0):
            parts += [np.ones(h), np.zeros(h)]
        d = h
    cols = []
    for width, scheme, value in heads:
        if scheme == "zeros":
            cols.append(np.zeros((d, width)))
        elif scheme == "normal":
            cols.append(rng.normal(0.0, value, (d, width)))
        elif scheme == "lecun":
            cols.append(_truncated_normal(rng, (d, width), np.sqrt(1.0 / d)))
        else:
            cols.append(_truncated_normal(rng, (d, width), np.sqrt(value / d)))
    parts += [np.concatenate(cols, axis=1), np.zeros(sum(w for w, _, _ in heads))]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def policy_heads(kind, A):
    """[mean | std] columns (policy.py:61-63, :85-87, :119-121)"""
    if kind == "fastsac":
        return [(A, "zeros", 0.0), (A, "zeros", 0.0)]
    if kind == "fasttd3":
        return [(A, "normal", 0.01), (A, "zeros", 0.0)]
    return [(A, "variance", 1e-4), (A, "variance", 1e-4)]


def critic_heads(kind, NA):
    """critic.py:42, :60, :88"""
    return [(NA, "variance", 1e-5)] if kind == "mpo" else [(NA, "lecun", 0.0)]


class FastMPO(FastOffPolicyLoop):
    _NAME = "fastmpo.hip"

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        if alg.device != "gpu":
            raise ValueError("fastmpo.hip runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        if int(alg.nr_parallel_seeds) > 1:                                                      # fastmpo.py:112-113
            raise ValueError("Parallel seeds are not supported yet.")
        if alg.policy_network_type not in KINDS or alg.critic_network_type not in KINDS:
            raise ValueError("fastmpo.hip: policy_network_type / critic_network_type must be one of " + ", ".join(KINDS))
        if alg.action_rescaling not in RESCALING:
            raise ValueError("fastmpo.hip: action_rescaling must be one of " + ", ".join(RESCALING))
        if bool(alg.clipped_double_q_learning) and not bool(alg.dual_critic):                  # default_config.py:54
            raise ValueError("fastmpo.hip: clipped_double_q_learning is only possible if dual_critic is True")
        if int(alg.learning_starts) < int(alg.n_steps):                                         # fastmpo.py:109-110
            raise ValueError("The replay buffer must at least be filled with n_steps transitions before learning starts.")
        self.nr_envs = int(config.environment.nr_envs)
        self.logging_frequency = int(alg.logging_frequency)
        self.evaluation_and_save_frequency = int(alg.evaluation_and_save_frequency)
        self.total_timesteps = int(alg.total_timesteps)
        if self.evaluation_and_save_frequency == -1:                                            # fastmpo.py:90-91
            self.evaluation_and_save_frequency = self.nr_envs * (self.total_timesteps // self.nr_envs)
        if self.evaluation_and_save_frequency % self.nr_envs != 0:                              # fastmpo.py:100-107
            raise ValueError("Evaluation and save frequency must be a multiple of nr envs.")
        if self.logging_frequency % self.nr_envs != 0:
            raise ValueError("Logging frequency must be a multiple of nr envs.")
        if self.evaluation_and_save_frequency % self.logging_frequency != 0:
            raise ValueError("Evaluation and save frequency must be a multiple of logging frequency.")
        import torch
        from rlx_amd.hip import Ctx, FastMpoHparams, fastmpo_desc
        from rlx_amd.hip import lib as hiplib
        if train_env.general_properties.data_interface_type != DataInterfaceType.TORCH:
            raise ValueError("fastmpo.hip needs a TORCH data-interface environment")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("fastmpo.hip is single-GPU (its normaliser statistics and gradients are not all-reduced)")
        except ImportError:
            pass
        self.torch, self.hiplib = torch, hiplib
        self.config, self.train_env, self.eval_env, self.writer = config, train_env, eval_env, writer
        self.save_model = config.runner.save_model
        self.save_path = os.path.join(run_path, "models")
        self.seed = config.environment.seed
        self.lrs = tuple(float(alg[k]) for k in ("critic_learning_rate", "policy_learning_rate", "dual_learning_rate"))
        self.anneal = tuple(bool(alg[k]) for k in ("anneal_critic_learning_rate", "anneal_policy_learning_rate", "anneal_dual_learning_rate"))
        self.batch_size, self.capacity = int(alg.batch_size), int(alg.buffer_size_per_env)
        self.learning_starts, self.n_steps = int(alg.learning_starts), int(alg.n_steps)
        self.G, self.P = int(alg.nr_critic_updates_per_policy_update), int(alg.nr_policy_updates_per_step)
        self.evaluation_active = bool(alg.evaluation_active)
        self.online_acting = bool(alg.collect_data_with_online_policy)
        self.obs_norm, self.norm_eps = bool(alg.enable_observation_normalization), float(alg.normalizer_epsilon)
        self.scheme = 1 if alg.threefry_partitionable else 0
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.ctx = Ctx(self.device.index or 0)
        self.sink = MetricSink(rlx_logger, writer, console=config.runner.track_console, tensorboard=config.runner.track_tb,
                               wandb=config.runner.track_wandb, rank=0)
        O = int(np.prod(train_env.single_observation_space.shape))
        A = int(np.prod(train_env.single_action_space.shape))
        self.obs_dim, self.act_dim = O, A
        from rlx_amd.algorithms.ppo.hip.ppo import PPO as _PPO
        pidx, cidx = _PPO._observation_indices(train_env, O)            # policy.py:18, critic.py:14
        self.obs_select = pidx is not None
        Op, Oc = (len(pidx), len(cidx)) if self.obs_select else (O, O)
        self.pidx = torch.from_numpy(pidx).to(self.device) if self.obs_select else None
        self.cidx = torch.from_numpy(cidx).to(self.device) if self.obs_select else None
        # get_processed_action's operands (policy.py:28-37); spaces without center / scale: mid-point, 1
        sp = train_env.single_action_space
        low, high = (np.asarray(getattr(sp, k), np.float32).reshape(-1) for k in ("low", "high"))
        center = np.asarray(getattr(sp, "center", 0.5 * (low + high)), np.float32).reshape(-1)
        scale = np.asarray(getattr(sp, "scale", np.ones(A)), np.float32).reshape(-1)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
        self.act_low, self.act_high = t(low), t(high)
        self.action_scale = t(np.maximum(np.abs(low - center), np.abs(high - center)) / scale)
        pk, ck, NA = str(alg.policy_network_type), str(alg.critic_network_type), int(alg.nr_atoms)
        self.E = 2 if bool(alg.dual_critic) else 1
        self.desc = fastmpo_desc(Op, Oc, A, NA, self.E == 2, pk, ck)    # the reference's widths (policy.py, critic.py)
        rng = np.random.default_rng(self.seed)
        self.pparams = t(init_params(rng, pk, Op, tuple(self.desc.policy_hidden), policy_heads(pk, A)))
        self.qparams = t(np.concatenate([init_params(rng, ck, Oc + A, tuple(self.desc.critic_hidden), critic_heads(ck, NA))
                                         for _ in range(self.E)]))
        assert self.pparams.numel() == self.ctx.fastmpo_param_count(self.desc, 0)
        assert self.qparams.numel() == self.E * self.ctx.fastmpo_param_count(self.desc, 1)
        self.tpparams, self.tqparams = self.pparams.clone(), self.qparams.clone()               # fastmpo.py:156, :166
        self.duals = t(np.array([alg.init_log_eta] + [alg.init_log_alpha_mean] * A + [alg.init_log_alpha_stddev] * A +
                                [alg.init_log_penalty_temperature], np.float32))                # dual_variables.py
        z = torch.zeros_like
        self.pm, self.pv, self.qm, self.qv, self.dm, self.dv = (z(x) for x in (self.pparams, self.pparams, self.qparams, self.qparams,
                                                                               self.duals, self.duals))
        self.opt_counts = (0, 0, 0)                                     # critic, policy, dual optimiser steps
        self.key = hiplib.prng_key(self.seed)
        if self.obs_norm:                                               # fastmpo.py:182-188
            self.norm_mean, self.norm_var, self.norm_std = (torch.zeros(O, device=self.device), torch.ones(O, device=self.device),
                                                            torch.ones(O, device=self.device))
            self.norm_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.hp = hp = FastMpoHparams()
        for k in ("gamma", "v_min", "v_max", "max_grad_norm", "policy_weight_decay", "critic_weight_decay", "dual_weight_decay", "critic_tau",
                  "policy_tau", "epsilon_non_parametric", "epsilon_parametric_mu", "epsilon_parametric_sigma", "epsilon_penalty",
                  "policy_init_scale", "policy_min_scale", "float_epsilon", "min_log_temperature", "min_log_alpha"):
            setattr(hp, k, float(alg[k]))
        hp.adam_b1, hp.adam_b2, hp.adam_eps = float(alg.adam_beta1), float(alg.adam_beta2), 1e-8     # optax.adamw's eps
        hp.action_sampling_number, hp.action_clipping = int(alg.action_sampling_number), int(bool(alg.action_clipping))
        hp.action_rescaling = RESCALING.index(alg.action_rescaling)
        hp.clipped_double_q_learning = int(bool(alg.clipped_double_q_learning))
        hp.nr_critic_updates_per_policy_update, hp.nr_policy_updates_per_step = self.G, self.P
        self.horizon = getattr(train_env, "horizon", 1000)
        if self.save_model:
            os.makedirs(self.save_path, exist_ok=True)

    # ------------------------------------------------------------------ pieces
    def _alloc(self):
        t = self.torch
        N, O, A, cap = self.nr_envs, self.obs_dim, self.act_dim, self.capacity
        f = dict(device=self.device, dtype=t.float32)
        self.ring = (t.zeros(cap, N, O, **f), t.zeros(cap, N, O, **f), t.zeros(cap, N, A, **f), t.zeros(cap, N, **f), t.zeros(cap, N, **f),
                     t.zeros(cap, N, **f))                                # states, next_states, actions, rewards, dones, truncations
        self.pos = self.size = 0
        T = self.P * self.G * self.batch_size
        self.both = t.empty(2 * T, O, **f)                                # [states_all; next_states_all]: one normaliser merge
        self.total = (self.both[:T], self.both[T:], t.empty(T, A, **f)) + tuple(t.empty(T, **f) for _ in range(4))
        self.idx_t, self.idx_e = t.empty(T, dtype=t.int32, device=self.device), t.empty(T, dtype=t.int32, device=self.device)
        n = len(METRIC_NAMES)
        self.metrics, self.sum_m, self.n_met = t.zeros(n, **f), t.zeros(n, **f), 0

    def _act_buffers(self, n):
        bufs = self.__dict__.setdefault("_act_bufs", {})
        if n not in bufs:
            t = self.torch
            f = dict(device=self.device, dtype=t.float32)
            bufs[n] = (t.empty(n, self.obs_dim, **f), t.empty(n, self.act_dim, **f), t.empty(n, self.act_dim, **f))
        return bufs[n]

    def act_pair(self, state, deterministic=False, params=None):
        """normalise (statistics frozen) + mean + std eps -> (action for the ring, processed action)"""
        norm, action, processed = self._act_buffers(int(state.shape[0]))
        x = state.contiguous()
        if self.obs_norm:
            x = self.ctx.obs_norm_apply(x, self.norm_mean, self.norm_std, norm, self.norm_eps)
        mode = self.hp.action_rescaling
        low, high = (self.act_low, self.act_high) if mode == 1 else (self.action_scale, None) if mode == 2 else (None, None)
        self.key = self.ctx.fastmpo_act(self.desc, self.pparams if params is None else params, x, self.key, action, processed, self.hp, low,
                                        high, deterministic=deterministic, pidx=self.pidx, scheme=self.scheme)
        return action, processed

    def act(self, state, deterministic=False):
        """the action the env gets from the ONLINE policy (evaluation, test(): fastmpo.py:678-680)"""
        return self.act_pair(state, deterministic)[1]

    def learning_rates(self):
        """per optimiser step of the coming update: lr (1 - count nr_envs / total_timesteps) when annealed (fastmpo.py:126-146)"""
        def sched(i, count, n):
            c = count + np.arange(n)
            frac = 1.0 - (c * self.nr_envs) / self.total_timesteps if self.anneal[i] else np.ones(n)
            return (self.lrs[i] * frac).astype(np.float32)
        cc, pc, dc = self.opt_counts
        return sched(0, cc, self.P * self.G), sched(1, pc, self.P), sched(2, dc, self.P)

    def _patch_newest_truncation(self):
        """fastmpo.py:497-503 for n_steps == 1 (the sampler applies it itself for n_steps > 1): a full ring's newest row counts as
        truncated unless it is done"""
        if self.n_steps != 1 or self.size < self.capacity:
            return
        truncs = self.total[5]
        truncs.copy_(patch_newest_truncation(self.torch, self.idx_t, self.total[4], truncs, (self.pos - 1) % self.capacity))

    def optimize(self):
        """fastmpo.py:494-627 for one learning iteration"""
        T, B = self.idx_t.numel(), self.batch_size
        max_start = self.capacity if self.size >= self.capacity else max(1, self.size - self.n_steps + 1)       # :497-509
        ks = self.hiplib.threefry_split(self.key, 4, self.scheme)          # key, idx_key_t, idx_key_e, noise_key (:495)
        self.key, noise_key = ks[0], ks[3]
        self.ctx.sac_replay_draw(ks[1], T, max_start, self.nr_envs, self.idx_t, self.idx_e, self.scheme)
        self.ctx.fastsac_replay_sample(self.ring, self.n_steps, self.hp.gamma, self.pos, self.size, self.idx_t, self.idx_e, self.total)
        self._patch_newest_truncation()
        if self.obs_norm:                                                   # :550-567: one merge of the 2 T rows, then both halves
            self.ctx.obs_norm_update(self.both, self.norm_mean, self.norm_var, self.norm_std, self.norm_count)
            self.ctx.obs_norm_apply(self.both, self.norm_mean, self.norm_std, self.both, self.norm_eps)
        U = self.P * self.G
        batch = tuple(x.view(U, B, -1) if x.dim() == 2 else x.view(U, B) for x in self.total)
        nets = (self.pparams, self.pm, self.pv, self.tpparams, self.qparams, self.qm, self.qv, self.tqparams, self.duals, self.dm, self.dv)
        self.opt_counts = self.ctx.fastmpo_update(self.desc, nets, batch, noise_key, self.opt_counts, *self.learning_rates(), self.hp,
                                                  self.metrics, pidx=self.pidx, cidx=self.cidx, scheme=self.scheme)
        self.sum_m += self.metrics
        self.n_met += 1

    def _vector_step(self, state):
        action, proc = self.act_pair(state, params=self.pparams if self.online_acting else self.tpparams)
        next_state, reward, terminated, truncated, info = self.train_env.step(proc)
        done = terminated | truncated
        actual_next = self._final_next_state(next_state, done, info)                              # fastmpo.py:247
        self.replay_add(state, actual_next, action, reward, done.float(), truncated.float())     # fastmpo.py:246-253
        return next_state.clone()

    # ------------------------------------------------------------------ training loop (fastmpo.py:198-714)
    def train(self):
        self._alloc()
        env = self.train_env
        state, _ = env.reset()
        state = state.clone()
        for _ in range(self.learning_starts):                                                     # fastmpo.py:227-267
            state = self._vector_step(state)
        global_step = nr_episodes = 0
        last_log_time, last_log_step = time.time(), 0
        while global_step < self.total_timesteps:
            state = self._vector_step(state)
            self.optimize()
            global_step += self.nr_envs
            if global_step % self.logging_frequency == 0 or global_step >= self.total_timesteps:
                now = time.time()
                combined = {}
                if self.n_met:
                    m = (self.sum_m / self.n_met).cpu().tolist()                                 # one D2H per logging interval
                    if not all(np.isfinite(v) for v in m):
                        raise FloatingPointError("fastmpo.hip: non-finite loss / gradient norm since the last log " + str(m))
                    combined.update(dict(zip(METRIC_NAMES, m)))
                    self.sum_m.zero_()
                    self.n_met = 0
                if hasattr(env, "pop_episode_stats"):
                    n_done, mean_ret, mean_len = env.pop_episode_stats()
                    nr_episodes += n_done
                    if n_done:
                        combined.update({"rollout/episode_return": mean_ret, "rollout/episode_length": mean_len})
                combined.update({"steps/nr_env_steps": global_step, "steps/nr_policy_updates": self.opt_counts[1],
                                 "steps/nr_critic_updates": self.opt_counts[0], "steps/nr_episodes": nr_episodes,
                                 "time/sps": int((global_step - last_log_step) / max(now - last_log_time, 1e-9))})
                last_log_time, last_log_step = now, global_step
                if global_step % self.evaluation_and_save_frequency == 0:                         # fastmpo.py:670-709
                    if self.evaluation_active:
                        rets, lens = self.evaluate()
                        combined.update({"eval/episode_return": float(np.mean(rets)) if rets else float("nan"),
                                         "eval/episode_length": float(np.mean(lens)) if lens else float("nan")})
                    if self.save_model:
                        self.save()
                self.sink.write(global_step, combined)
                self.last_metrics = combined

    _STATE = ("pparams", "pm", "pv", "tpparams", "qparams", "qm", "qv", "tqparams", "duals", "dm", "dv")

    def save(self):
        """Native checkpoint: every network and target, the duals, all AdamW moments, the normaliser, the optimiser counts, the key
        and the algorithm config (the reference stores its three train states and the normaliser, fastmpo.py:706-709)."""
        path = os.path.join(self.save_path, "latest.model")
        state = {k: getattr(self, k).cpu().numpy() for k in self._STATE + (self._NORM_STATE if self.obs_norm else ())}
        np.savez(path + ".tmp.npz", opt_counts=np.asarray(self.opt_counts, np.int64), key=self.key,
                 config_algorithm=json.dumps(self.config.algorithm.to_dict()), **state)
        os.replace(path + ".tmp.npz", path)

    def load(config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)
        model = FastMPO(config, train_env, eval_env, run_path, writer)
        for k in FastMPO._STATE + (FastMPO._NORM_STATE if model.obs_norm else ()):
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        model.opt_counts = tuple(int(x) for x in ckpt["opt_counts"])
        model.key = ckpt["key"].astype(np.uint32)
        return model

    def general_properties():
        return GeneralProperties
