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
import numpy as np

from rlx_amd.algorithms.fast_offpolicy import FastOffPolicyLoop
from rlx_amd.algorithms.fastmpo.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.hip_model import TRUNC_NORMAL_STD, eval_means

KINDS = ("fastsac", "fasttd3", "mpo")
RESCALING = ("none", "normal", "fastsac")
CRITIC_METRICS = ("loss/q_loss", "q/q_mean", "q/q_max", "q/q_min", "lr/critic_learning_rate", "gradients/critic_grad_norm")
POLICY_METRICS = ("loss/actor_loss", "loss/loss_pg_mean", "loss/loss_pg_std", "loss/loss_kl_mean", "loss/loss_kl_std", "loss/dual_loss",
                  "loss/loss_alpha_mean", "loss/loss_alpha_std", "loss/loss_eta", "dual/eta", "dual/penalty_temperature", "dual/alpha_mean",
                  "dual/alpha_std", "kl/mean_kl_mean", "kl/mean_kl_std", "q/improvement_q_mean", "policy/std_min_mean",
                  "policy/std_max_mean", "lr/policy_learning_rate", "lr/dual_variables_learning_rate", "gradients/policy_grad_norm",
                  "gradients/dual_variables_grad_norm")
METRIC_NAMES = CRITIC_METRICS + POLICY_METRICS        # fastmpo.py:372-377, :595-596, :461-480, :624-627: rlx_fastmpo_update_f32's order


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
    _STATE = ("pparams", "pm", "pv", "tpparams", "qparams", "qm", "qv", "tqparams", "duals", "dm", "dv")
    _COUNTERS = ("opt_counts",)

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = self._read_flags(config, train_env, eval_env, run_path, writer)
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
        self.logging_frequency = int(alg.logging_frequency)
        self.evaluation_and_save_frequency = int(alg.evaluation_and_save_frequency)
        if self.evaluation_and_save_frequency == -1:                                            # fastmpo.py:90-91
            self.evaluation_and_save_frequency = self.nr_envs * (self.total_timesteps // self.nr_envs)
        if self.evaluation_and_save_frequency % self.nr_envs != 0:                              # fastmpo.py:100-107
            raise ValueError("Evaluation and save frequency must be a multiple of nr envs.")
        if self.logging_frequency % self.nr_envs != 0:
            raise ValueError("Logging frequency must be a multiple of nr envs.")
        if self.evaluation_and_save_frequency % self.logging_frequency != 0:
            raise ValueError("Evaluation and save frequency must be a multiple of logging frequency.")
        self.lrs = tuple(float(alg[k]) for k in ("critic_learning_rate", "policy_learning_rate", "dual_learning_rate"))
        self.anneal = tuple(bool(alg[k]) for k in ("anneal_critic_learning_rate", "anneal_policy_learning_rate", "anneal_dual_learning_rate"))
        self.batch_size, self.capacity = int(alg.batch_size), int(alg.buffer_size_per_env)
        self.learning_starts, self.n_steps = int(alg.learning_starts), int(alg.n_steps)
        self.G, self.P = int(alg.nr_critic_updates_per_policy_update), int(alg.nr_policy_updates_per_step)
        self.evaluation_active = bool(alg.evaluation_active)
        self.online_acting = bool(alg.collect_data_with_online_policy)
        self.obs_norm, self.norm_eps = bool(alg.enable_observation_normalization), float(alg.normalizer_epsilon)
        self._open_device()
        from rlx_amd.hip import FastMpoHparams, fastmpo_desc
        torch = self.torch
        A, Op, Oc = self.act_dim, self.policy_obs_dim, self.critic_obs_dim      # policy.py:18, critic.py:14
        self._action_bounds()                                           # get_processed_action's operands (policy.py:28-37)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
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
        self._alloc_normalizer()                                        # fastmpo.py:182-188
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

    # ------------------------------------------------------------------ pieces
    def _alloc(self):
        t, T = self.torch, self.P * self.G * self.batch_size
        f = self._alloc_ring(T)
        self.both = t.empty(2 * T, self.obs_dim, **f)                     # [states_all; next_states_all]: one normaliser merge
        self.total = (self.both[:T], self.both[T:]) + self.total[2:]
        n = len(METRIC_NAMES)
        self.metrics, self.sum_m, self.n_met = t.zeros(n, **f), t.zeros(n, **f), 0

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
        global_step = 0
        self._start_log()
        while global_step < self.total_timesteps:
            state = self._vector_step(state)
            self.optimize()
            global_step += self.nr_envs
            if global_step % self.logging_frequency == 0 or global_step >= self.total_timesteps:
                combined = {}
                if self.n_met:
                    combined.update(dict(zip(METRIC_NAMES, self._mean_metrics(self.sum_m))))        # one D2H per logging interval
                    self.sum_m.zero_()
                    self.n_met = 0
                self._episode_stats(combined)
                combined.update({"steps/nr_env_steps": global_step, "steps/nr_policy_updates": self.opt_counts[1],
                                 "steps/nr_critic_updates": self.opt_counts[0], "steps/nr_episodes": self.nr_episodes,
                                 "time/sps": self._sps(global_step)})
                if global_step % self.evaluation_and_save_frequency == 0:                         # fastmpo.py:670-709
                    if self.evaluation_active:
                        combined.update(eval_means(*self.evaluate()))
                    if self.save_model:
                        self.save()
                self._write_log(global_step, combined)

    def general_properties():
        return GeneralProperties
