"""`reppo.hip`: the REPPO training loop of rl_x/algorithms/reppo/pytorch/reppo.py:111-468 around the library's steps
(rl-x_amd/csrc/reppo.hip).

Per iteration: nr_steps rollout steps, each normaliser update on the raw state and normalisation (:260-261), acting (:262), env
step, normalisation of the actual next state without update (:318) and evaluate_next, written straight into step t's batch slot
(:319-328); the soft TD-lambda targets (:339); the old-policy snapshot AFTER the rollout (:346); ONE whole-update call over
nr_epochs x nr_minibatches minibatches from the reference's own permutation -- one persistent arange(batch) shuffled in place
every epoch by np.random.default_rng(seed) (:359-361), generated on the host and uploaded once per iteration; LinearLR per
iteration when enabled (:399-401).  Metrics stay on the device until the iteration's one host read.

What differs from the reference, on purpose: random numbers (torch's CUDA generator there; the library's counter RNG here), fp32
instead of bf16 autocast, parameters initialised from numpy with torch's defaults (Linear uniform +-1/sqrt(fan_in), RMSNorm 1,
zero_distribution from its erf formula, log of the initial coefficients) drawn from np.random.default_rng([seed, 1]) -- a stream
separate from the permutation generator."""
import math
import time

import numpy as np

from rlx_amd.algorithms.hip_model import HipModel, eval_means
from rlx_amd.algorithms.reppo.hip.general_properties import GeneralProperties

METRIC_NAMES = ("loss/critic_loss", "loss/auxiliary_loss", "q/q_mean", "q/explained_variance", "gradients/critic_grad_norm",
                "loss/policy_loss", "loss/entropy_coefficient_loss", "loss/kl_coefficient_loss", "entropy/entropy",
                "kl/kl_divergence", "entropy/entropy_coefficient", "kl/kl_coefficient", "q/policy_q_mean",
                "gradients/policy_grad_norm")      # the update's per-minibatch row (rlx_reppo_update_f32), reppo.py:382-397


def zero_distribution(nr_bins, v_min, v_max):
    """critic.py:50-53 in float32"""
    import torch
    bw = (v_max - v_min) / (nr_bins - 1)
    support = torch.linspace(v_min - bw / 2, v_max + bw / 2, nr_bins + 1, dtype=torch.float32)
    cdf = torch.erf(support / (np.sqrt(2) * bw * 0.75))
    return ((cdf[1:] - cdf[:-1]) / (cdf[-1] - cdf[0])).numpy()


def init_params(rng, Op, Oc, A, Hp, Hc, nr_bins, v_min, v_max, init_entropy_coefficient, init_kl_coefficient):
    """(policy flat, critic flat) in the layouts of include/rlx_hip.h (rlx_reppo_desc), float32"""
    def lin(i, o, rms):
        b = 1.0 / np.sqrt(i)
        parts = [rng.uniform(-b, b, i * o), rng.uniform(-b, b, o)]
        return parts + [np.ones(o)] if rms else parts
    p = lin(Op, Hp, True) + lin(Hp, Hp, True) + lin(Hp, 2 * A, False)
    p += [np.array([math.log(init_entropy_coefficient), math.log(init_kl_coefficient)])]
    q = lin(Oc + A, Hc, True) + lin(Hc, Hc, False) + lin(Hc, Hc, True) + lin(Hc, nr_bins, False) + lin(Hc, Hc, True)
    q += lin(Hc, Hc + 1, False) + [zero_distribution(nr_bins, v_min, v_max)]
    return np.concatenate(p).astype(np.float32), np.concatenate(q).astype(np.float32)


class REPPO(HipModel):
    _NAME = "reppo.hip"
    _FILE = "best.model"
    _STATE = ("pparams", "pm", "pv", "qparams", "qm", "qv", "norm_mean", "norm_var", "norm_count")
    _NORM_STATE = ()                # the float32-count normaliser below is part of _STATE whether or not it is applied
    _COUNTERS = ("opt_count", "nr_iterations_done")

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = self._read_flags(config, train_env, eval_env, run_path, writer)
        self.learning_rate, self.anneal_learning_rate = float(alg.learning_rate), bool(alg.anneal_learning_rate)
        self.nr_steps, self.nr_epochs, self.nr_minibatches = int(alg.nr_steps), int(alg.nr_epochs), int(alg.nr_minibatches)
        self.evaluation_frequency, self.evaluation_episodes = int(alg.evaluation_frequency), int(alg.evaluation_episodes)
        self.obs_norm = bool(alg.normalize_observation)
        self.batch_size = self.nr_envs * self.nr_steps
        self.nr_rollout_updates = self.total_timesteps // self.batch_size
        if self.nr_rollout_updates == 0:                                                          # reppo.py:65-70
            raise ValueError("The total number of timesteps must contain at least one rollout batch.")
        if self.batch_size % self.nr_minibatches != 0:
            raise ValueError("The rollout batch size must be divisible by the number of minibatches.")
        if self.evaluation_frequency != -1 and self.evaluation_frequency % self.batch_size != 0:
            raise ValueError("Evaluation frequency must be a multiple of the number of steps and environments.")
        self._open_device()
        from rlx_amd.hip import ReppoHparams, reppo_desc
        torch = self.torch
        O, A, Op, Oc = self.obs_dim, self.act_dim, self.policy_obs_dim, self.critic_obs_dim     # policy.py:13, critic.py:11
        sp = train_env.single_action_space                                     # policy.py:30-39
        low, high = (np.asarray(getattr(sp, k), np.float32).reshape(-1) for k in ("low", "high"))
        if hasattr(sp, "center") and hasattr(sp, "scale"):
            c, s = np.asarray(sp.center, np.float32).reshape(-1), np.asarray(sp.scale, np.float32).reshape(-1)
            low, high = (low - c) / s, (high - c) / s
        self.act_low, self.act_high = (torch.from_numpy(x.copy()).to(self.device) for x in (low, high))
        self.desc = reppo_desc(Op, Oc, A, int(alg.policy_hidden_dim), int(alg.critic_hidden_dim), int(alg.nr_bins))
        p, q = init_params(np.random.default_rng([int(self.seed), 1]), Op, Oc, A, int(alg.policy_hidden_dim), int(alg.critic_hidden_dim),
                           int(alg.nr_bins), float(alg.v_min), float(alg.v_max), float(alg.init_entropy_coefficient),
                           float(alg.init_kl_coefficient))
        self.pparams, self.qparams = torch.from_numpy(p).to(self.device), torch.from_numpy(q).to(self.device)
        self.old_pparams = self.pparams.clone()
        z = torch.zeros_like
        self.pm, self.pv, self.qm, self.qv = z(self.pparams), z(self.pparams), z(self.qparams), z(self.qparams)
        self.opt_count = 0
        self.nr_iterations_done = 0
        self.rng = np.random.default_rng(self.seed)                            # reppo.py:84: the permutation generator
        self.norm_mean, self.norm_var = torch.zeros(O, device=self.device), torch.ones(O, device=self.device)
        self.norm_count = torch.full((1,), 1e-4, device=self.device)            # observation_normalizer.py:11
        self.hp = ReppoHparams()
        for k in ("gamma", "gae_lambda", "v_min", "v_max", "kl_bound", "policy_min_std", "auxiliary_loss_coefficient", "max_grad_norm"):
            setattr(self.hp, k, float(alg[k]))
        self.hp.target_entropy = A * float(alg.target_entropy_multiplier)       # reppo.py:63
        self.hp.adam_b1, self.hp.adam_b2, self.hp.adam_eps = 0.9, 0.999, 1e-8   # torch.optim.Adam defaults (reppo.py:97-98)
        self.hp.nr_kl_samples = int(alg.nr_kl_samples)
        self.best_mean_return = -np.inf

    # ------------------------------------------------------------------ pieces
    def current_lr(self, iteration):
        """LinearLR(start 1, end 0, total_iters = nr_rollout_updates), stepped once per iteration (reppo.py:100-102, :399-404)"""
        if not self.anneal_learning_rate:
            return self.learning_rate
        return self.learning_rate * max(1.0 - min(iteration, self.nr_rollout_updates) / self.nr_rollout_updates, 0.0)

    def normalize(self, obs, out, update):
        """ObservationNormalizer.update / normalize (observation_normalizer.py:14-34)"""
        if not self.obs_norm:
            return out.copy_(obs)
        if update:
            self.ctx.reppo_obs_norm_update(obs, self.norm_mean, self.norm_var, self.norm_count)
        return self.ctx.reppo_obs_norm_apply(obs, self.norm_mean, self.norm_var, out)

    def act(self, state, deterministic=False):
        """normalize (no update) + rollout_act / deterministic_action -> the env's action (evaluation, test())"""
        x, action, processed = self._act_buffers(int(state.shape[0]))
        self.normalize(state.contiguous(), x, False)
        self.key = self.ctx.reppo_act(self.desc, self.pparams, x, self.key, action, processed, self.act_low, self.act_high, self.hp,
                                      deterministic, pidx=self.pidx, scheme=self.scheme)
        return processed

    def _alloc(self):
        t, T, N = self.torch, self.nr_steps, self.nr_envs
        f = dict(device=self.device, dtype=t.float32)
        self.b_states, self.b_actions = t.zeros(T, N, self.obs_dim, **f), t.zeros(T, N, self.act_dim, **f)
        self.b_rewards, self.b_soft, self.b_nv, self.b_term, self.b_trunc, self.b_targets = (t.zeros(T, N, **f) for _ in range(6))
        self.b_nf = t.zeros(T, N, self.desc.critic_hidden, **f)
        self.b_next = t.empty(N, self.obs_dim, **f)
        self.b_proc = t.empty(N, self.act_dim, **f)
        self.metrics = t.zeros(self.nr_epochs * self.nr_minibatches, len(METRIC_NAMES), **f)
        self.batch_indices = np.arange(self.batch_size)

    def rollout_step(self, state, t):
        """reppo.py:260-328 for step t -> (next state, done count this step)"""
        env = self.train_env
        s = self.b_states[t]
        self.normalize(state.contiguous(), s, True)
        self.key = self.ctx.reppo_act(self.desc, self.pparams, s, self.key, self.b_actions[t], self.b_proc, self.act_low, self.act_high,
                                      self.hp, pidx=self.pidx, scheme=self.scheme)
        next_state, reward, terminated, truncated, info = env.step(self.b_proc)
        done = terminated | truncated
        actual = next_state
        if "final_observation" in info and self.torch.is_tensor(info["final_observation"]):     # reppo.py:293-296
            mask = info.get("_final_observation", done).bool()
            actual = self.torch.where(mask.unsqueeze(-1), info["final_observation"], next_state)
        self.b_rewards[t].copy_(reward)
        self.b_term[t].copy_(terminated)
        self.b_trunc[t].copy_(truncated)
        self.normalize(actual.contiguous(), self.b_next, False)
        self.key = self.ctx.reppo_evaluate_next(self.desc, self.pparams, self.qparams, self.b_next, self.b_rewards[t], self.key,
                                                self.b_nf[t], self.b_nv[t], self.b_soft[t], self.hp, self.pidx, self.cidx, self.scheme)
        return next_state.clone()

    def permutation(self):
        """reppo.py:359-361: the persistent index array shuffled in place every epoch -> int32 [nr_epochs, batch]"""
        perm = np.empty((self.nr_epochs, self.batch_size), np.int32)
        for e in range(self.nr_epochs):
            self.rng.shuffle(self.batch_indices)
            perm[e] = self.batch_indices
        return perm

    def optimize(self):
        """targets, old-policy snapshot, one whole-update call (reppo.py:337-405) -> the iteration's mean metrics (host)"""
        t = self.torch
        self.ctx.reppo_td_lambda(self.b_soft, self.b_nv, self.b_term, self.b_trunc, self.hp.gamma, self.hp.gae_lambda, self.b_targets)
        self.old_pparams.copy_(self.pparams)
        perm = t.from_numpy(self.permutation()).to(self.device)
        B = self.batch_size
        batch = (self.b_states.view(B, -1), self.b_actions.view(B, -1), self.b_rewards.view(B), self.b_targets.view(B),
                 self.b_nf.view(B, -1), self.b_term.view(B), self.b_trunc.view(B))
        lr = self.current_lr(self.nr_iterations_done)
        self.key, self.opt_count = self.ctx.reppo_update(self.desc, self.pparams, self.pm, self.pv, self.old_pparams, self.qparams, self.qm,
                                                         self.qv, batch, perm, self.nr_minibatches, self.key, self.opt_count, lr, self.hp,
                                                         self.metrics, pidx=self.pidx, cidx=self.cidx, scheme=self.scheme)
        self.nr_iterations_done += 1
        out = dict(zip(METRIC_NAMES, self._finite(self.metrics.mean(0).cpu().tolist(), "in this iteration")))    # the one host read
        out["lr/learning_rate"] = lr if not self.anneal_learning_rate else self.current_lr(self.nr_iterations_done)
        return out

    # ------------------------------------------------------------------ training loop (reppo.py:111-468)
    def train(self):
        self._alloc()
        state, _ = self.train_env.reset()
        state = state.clone()
        global_step = 0
        self._start_log()
        prev_end = None
        while global_step < self.total_timesteps:
            start = time.time()
            for t in range(self.nr_steps):
                state = self.rollout_step(state, t)
                global_step += self.nr_envs
            acting_end = time.time()
            metrics = self.optimize()
            optimizing_end = time.time()
            if self.evaluation_frequency != -1 and global_step % self.evaluation_frequency == 0:
                metrics.update(eval_means(*self.evaluate(self.evaluation_episodes)))
            n_done, mean_ret = self._episode_stats(metrics)
            if n_done and self.save_model and mean_ret > self.best_mean_return:
                self.best_mean_return = mean_ret
                self.save()
            end = time.time()
            metrics.update({"time/acting_time": acting_end - start, "time/optimizing_time": optimizing_end - acting_end,
                            "steps/nr_env_steps": global_step, "steps/nr_updates": self.opt_count, "steps/nr_episodes": self.nr_episodes})
            if prev_end is not None:                                       # per iteration, end to end: absent from the first
                metrics["time/sps"] = int(self.batch_size / max(end - prev_end, 1e-9))
            prev_end = end
            self._write_log(global_step, metrics)

    def test(self, episodes):
        return self.evaluate(episodes)[0]

    def _after_load(self):
        self.old_pparams.copy_(self.pparams)

    def general_properties():
        return GeneralProperties
