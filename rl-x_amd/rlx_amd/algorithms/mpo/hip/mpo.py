"""`mpo.hip`: the MPO training loop of rl_x/algorithms/mpo/pytorch/mpo.py:272-420 around the library's update (rl-x_amd/csrc/mpo.hip).

Per vector step: before `learning_starts` env steps a uniform random action in the action space, mapped back to [-1, 1] for the ring
(:298-300); after it the env actor's sample on the normalised state (:302-305).  The env gets the processed action, the ring the
UNclipped one and the actual next state (final observation where an episode ended, :309-313).  Every `actor_update_period`
iterations env actor <- target actor (:345-346); every `optimize_every_n_steps` iterations one ring sample, the normaliser updated on
the sampled states and then on the next states (:351-353), ONE rlx_mpo_update_f32 call, and every `target_network_update_period`
updates target <- online for both networks (:384-386).  LinearLR per update when enabled (:105-109, :412-416).  Evaluation and test()
use the ONLINE actor's deterministic action (:431, :581).  Metrics stay on the device until a log's one host read.

The ring, its sampling and the normaliser are FastTD3's / FastSAC's (mpo/pytorch/replay_buffer.py is byte-identical to FastTD3's,
observation_normalizer.py to FastSAC's): rlx_amd/algorithms/fast_offpolicy.py.  What differs from the reference, on purpose: random
numbers (torch / numpy generators there; the library's counter RNG here for the action and update noise and the replay indices,
numpy for the warm-up actions), fp32 instead of bf16 autocast, parameters initialised from numpy with the reference's own schemes
(uniform +-sqrt(3 / fan_in) 0.333 hidden layers with zero bias, LayerNorm 1 / 0, heads N(0, std^2) with policy.py:61-68's variance
scaling)."""
import numpy as np

from rlx_amd.algorithms.fast_offpolicy import FastOffPolicyLoop
from rlx_amd.algorithms.hip_model import TRUNC_NORMAL_STD, eval_means
from rlx_amd.algorithms.mpo.hip.general_properties import GeneralProperties
from rlx_amd.environments.data_interface_type import DataInterfaceType

METRIC_NAMES = ("loss/critic_loss", "loss/actor_loss", "loss/dual_loss", "loss/loss_eta", "loss/loss_alpha", "q/current_q_mean",
                "dual/eta", "dual/penalty_temperature", "dual/alpha_mean", "dual/alpha_std", "kl/mean_kl_mean", "kl/mean_kl_std",
                "gradients/actor_grad_norm", "gradients/critic_grad_norm", "gradients/dual_grad_norm", "policy/std_min_mean",
                "policy/std_max_mean")      # mpo.py:389-407, the order of rlx_mpo_update_f32's metrics


def init_params(rng, in_dim, H, out_dim, head_std):
    """flat layout of include/rlx_hip.h (rlx_mpo_desc): uniform_scaling_layer_init (policy.py:54-58) for the three hidden Linears,
    LayerNorm weight 1 / bias 0, the head layer_init(std=head_std, variance_scaling=True) (policy.py:61-68; trunc_normal_'s +-2
    bounds are far outside these widths)"""
    parts, d = [], in_dim
    for li in range(3):
        bound = np.sqrt(3.0 / d) * 0.333
        parts += [rng.uniform(-bound, bound, (d, H)), np.zeros(H)]
        if li == 0:
            parts += [np.ones(H), np.zeros(H)]
        d = H
    std = np.sqrt(head_std / H) / TRUNC_NORMAL_STD
    parts += [rng.normal(0.0, std, (H, out_dim)), np.zeros(out_dim)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


class MPO(FastOffPolicyLoop):
    _NAME = "mpo.hip"
    _FILE = "best.model"
    _STATE = ("pparams", "pm", "pv", "tpparams", "qparams", "qm", "qv", "tqparams", "env_pparams", "duals", "dm", "dv")
    _COUNTERS = ("nr_updates",)

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = self._read_flags(config, train_env, eval_env, run_path, writer)
        self.agent_lr, self.dual_lr = float(alg.agent_learning_rate), float(alg.dual_learning_rate)
        self.anneal_agent, self.anneal_dual = bool(alg.anneal_agent_learning_rate), bool(alg.anneal_dual_learning_rate)
        self.learning_starts, self.batch_size, self.n_steps = int(alg.learning_starts), int(alg.batch_size), int(alg.n_steps)
        self.capacity = int(max(1, int(alg.buffer_size) // self.nr_envs))                      # mpo.py:272
        self.actor_update_period, self.target_period = int(alg.actor_update_period), int(alg.target_network_update_period)
        self.optimize_every = int(alg.optimize_every_n_steps)
        self.logging_frequency, self.evaluation_frequency = int(alg.logging_frequency), int(alg.evaluation_frequency)
        self.evaluation_episodes = int(alg.evaluation_episodes)
        self.obs_norm = bool(alg.enable_observation_normalization)
        self._open_device(torch_env_only=False)
        from rlx_amd.hip import MpoHparams, mpo_desc
        torch = self.torch
        self.numpy_env = train_env.general_properties.data_interface_type == DataInterfaceType.NUMPY
        A, Op, Oc = self.act_dim, self.policy_obs_dim, self.critic_obs_dim              # policy.py:13, q_network.py:10
        self.low_np, self.high_np = self._action_bounds()
        H, NA = int(alg.nr_hidden_units), int(alg.nr_atoms)
        self.desc = mpo_desc(Op, Oc, A, H, NA)
        rng = np.random.default_rng(self.seed)
        self.rng = np.random.default_rng([int(self.seed), 1])                       # the warm-up actions
        t = lambda a: torch.from_numpy(a).to(self.device)
        self.pparams = t(init_params(rng, Op, H, 2 * A, 1e-4))                       # policy.py:48-49
        self.qparams = t(init_params(rng, Oc + A, H, NA, 1e-5))                      # q_network.py:36
        self.tpparams, self.tqparams, self.env_pparams = self.pparams.clone(), self.qparams.clone(), self.pparams.clone()
        self.duals = t(np.array([alg.init_log_eta] + [alg.init_log_alpha_mean] * A + [alg.init_log_alpha_stddev] * A +
                                [alg.init_log_penalty_temperature], np.float32))    # dual_variables.py:7-10
        z = torch.zeros_like
        self.pm, self.pv, self.qm, self.qv, self.dm, self.dv = (z(x) for x in (self.pparams, self.pparams, self.qparams, self.qparams,
                                                                               self.duals, self.duals))
        self.nr_updates = 0
        self._alloc_normalizer()
        self.hp = hp = MpoHparams()
        for k in ("gamma", "v_min", "v_max", "max_grad_norm", "epsilon_non_parametric", "epsilon_parametric_mu", "epsilon_parametric_sigma",
                  "epsilon_penalty", "policy_init_scale", "policy_min_scale", "float_epsilon", "min_log_temperature", "min_log_alpha"):
            setattr(hp, k, float(alg[k]))
        hp.adam_b1, hp.adam_b2, hp.adam_eps = 0.9, 0.999, 1e-8                      # torch.optim.Adam defaults (mpo.py:101-103)
        hp.action_sampling_number = int(alg.action_sampling_number)
        hp.action_clipping, hp.action_rescaling = int(bool(alg.action_clipping)), int(bool(alg.action_rescaling))
        self.best_mean_return = -np.inf

    # ------------------------------------------------------------------ pieces
    def _alloc(self):
        t, f = self.torch, self._alloc_ring(self.batch_size)
        self.metrics, self.sum_m, self.n_met = t.zeros(17, **f), t.zeros(17, **f), 0

    def _dev(self, x, dtype=None):
        t = self.torch
        x = x if t.is_tensor(x) else t.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return x.to(self.device, dtype or t.float32).contiguous()

    def act_pair(self, state, deterministic=False, params=None):
        """normalize(update=False) + sample_action / get_deterministic_action -> (action for the ring, processed action), on the device"""
        norm, action, processed = self._act_buffers(int(state.shape[0]))
        x = self.normalize(self._dev(state), norm, False)
        low, high = (self.act_low, self.act_high) if self.hp.action_rescaling else (None, None)
        self.key = self.ctx.mpo_act(self.desc, self.pparams if params is None else params, x, self.key, action, processed, self.hp, low, high,
                                    deterministic=deterministic, pidx=self.pidx, scheme=self.scheme)
        return action, processed

    def _to_env(self, x):
        return x.cpu().numpy() if self.numpy_env else x

    def act(self, state, deterministic=False):
        """the action the env gets: the ONLINE actor's (evaluation, test(): mpo.py:431, :581)"""
        return self._to_env(self.act_pair(state, deterministic)[1])

    def optimize(self):
        """mpo.py:350-386 for one iteration"""
        self.sample()
        s, s2 = self.total[0], self.total[1]
        self.normalize(s, s, True)
        self.normalize(s2, s2, True)
        agent_lr, dual_lr = self.agent_lr, self.dual_lr
        total = max((self.total_timesteps - self.learning_starts) // self.nr_envs, 1)
        f = max(1.0 - min(self.nr_updates, total) / total, 0.0)                           # LinearLR(1 -> 0), stepped per update
        agent_lr, dual_lr = agent_lr * (f if self.anneal_agent else 1.0), dual_lr * (f if self.anneal_dual else 1.0)
        nets = (self.pparams, self.pm, self.pv, self.tpparams, self.qparams, self.qm, self.qv, self.tqparams, self.duals, self.dm, self.dv)
        self.key = self.ctx.mpo_update(self.desc, nets, self.total, self.key, self.nr_updates + 1, agent_lr, dual_lr, self.hp, self.metrics,
                                       pidx=self.pidx, cidx=self.cidx, scheme=self.scheme)
        self.nr_updates += 1
        if self.nr_updates % self.target_period == 0:
            self.tpparams.copy_(self.pparams)
            self.tqparams.copy_(self.qparams)
        self.sum_m += self.metrics
        self.n_met += 1

    # ------------------------------------------------------------------ training loop (mpo.py:272-500)
    def train(self):
        t = self.torch
        self._alloc()
        env = self.train_env
        state, _ = env.reset()
        state = self._dev(state)
        global_step = 0
        self._start_log()
        returns = []
        while global_step < self.total_timesteps:
            if global_step < self.learning_starts:                                            # mpo.py:298-300
                proc = self.rng.uniform(self.low_np, self.high_np, (self.nr_envs, self.act_dim)).astype(np.float32)
                action = self._dev((proc - self.low_np) / (self.high_np - self.low_np) * 2.0 - 1.0)
                proc = proc if self.numpy_env else self._dev(proc)
            else:
                action, proc = self.act_pair(state, params=self.env_pparams)
                proc = self._to_env(proc)
            next_state, reward, terminated, truncated, info = env.step(proc)
            next_state = self._dev(next_state)
            term, trunc = self._dev(terminated, t.bool), self._dev(truncated, t.bool)
            done = term | trunc
            actual_next = self._final_next_state(next_state, done, info)
            self.replay_add(state, actual_next, action, self._dev(reward), done.float(), trunc.float())
            if self.numpy_env and bool(np.any(np.asarray(terminated) | np.asarray(truncated))):
                ret = info.get("episode_return") if isinstance(info, dict) else None
                if ret is not None:
                    returns.extend(np.asarray(ret)[np.asarray(terminated) | np.asarray(truncated)].tolist())
            state = next_state
            global_step += self.nr_envs
            iteration = global_step // self.nr_envs
            started = global_step > self.learning_starts
            if started and iteration % self.actor_update_period == 0:                          # mpo.py:345-346
                self.env_pparams.copy_(self.tpparams)
            if started and iteration % self.optimize_every == 0:
                self.optimize()
            if self.evaluation_frequency != -1 and global_step % self.evaluation_frequency == 0:
                self.last_eval = eval_means(*self.evaluate())
            if global_step % self.logging_frequency == 0 or global_step >= self.total_timesteps:
                combined = {}
                if hasattr(env, "pop_episode_stats"):
                    self._episode_stats(combined)
                elif returns:
                    self.nr_episodes += len(returns)
                    combined["rollout/episode_return"] = float(np.mean(returns))
                if self.save_model and returns and float(np.mean(returns)) > self.best_mean_return and self.n_met:
                    self.best_mean_return = float(np.mean(returns))
                    self.save()
                returns = []
                combined.update(getattr(self, "last_eval", {}))
                combined.update({"steps/nr_env_steps": global_step, "steps/nr_updates": self.nr_updates,
                                 "steps/nr_episodes": self.nr_episodes, "time/sps": self._sps(global_step)})
                if self.n_met:
                    combined.update(dict(zip(METRIC_NAMES, self._mean_metrics(self.sum_m))))        # one D2H per logging interval
                    self.sum_m.zero_()
                    self.n_met = 0
                self._write_log(global_step, combined)

    def evaluate(self):
        """`horizon` deterministic steps of the online actor on the eval env -> (episode returns, lengths); NUMPY or TORCH env"""
        env = self.eval_env
        shared = env is self.train_env
        if shared and not hasattr(env, "snapshot"):
            raise ValueError("mpo.hip: evaluation on the training env needs env.snapshot()/restore(); "
                             "set environment.copy_train_env_for_eval=False")
        snap = env.snapshot() if shared else None
        try:
            state, _ = env.reset()
            ne = int(np.shape(state)[0])
            ep_ret, ep_len = np.zeros(ne), np.zeros(ne, np.int64)
            rets, lens = [], []
            for _ in range(int(self.horizon)):
                state, reward, terminated, truncated, _ = env.step(self.act(state, deterministic=True))
                host = lambda x: x.cpu().numpy() if self.torch.is_tensor(x) else np.asarray(x)
                ep_ret += host(reward)
                ep_len += 1
                done = host(terminated) | host(truncated)
                if done.any():
                    rets.extend(ep_ret[done].tolist())
                    lens.extend(ep_len[done].tolist())
                    ep_ret[done], ep_len[done] = 0.0, 0
            return rets, lens
        finally:
            if shared:
                env.restore(snap)

    def general_properties():
        return GeneralProperties
