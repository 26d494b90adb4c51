"""redq.hip -- REDQ whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/redq.hip).

The reference's REDQ (rl_x/algorithms/redq/flax/redq.py) is its SAC host loop with an ensemble of scalar critics and a high
update-to-data `update`: policy.py is sac/flax's file, acting (redq.py:134-140), the uniform warm-up (:298-300) and the replay ring
are the same.  This class therefore derives from `sac.hip`'s (through EnsembleSAC, what it shares with tqc.hip) and keeps its
acting, warm-up actions, ring, `_host_indices`, evaluation and `test`.  What it replaces: the critics -- ensemble_size independent
nets with one output each (critic.py:17-53), flat and back to back -- the sampling of q_update_steps batches at once
(replay_buffer.py:30-38), the update call (rlx_redq_update_f32: q_update_steps critic steps, then one policy / entropy step), the
two optimizer counters with their two schedules (redq.py:82-98) and the checkpoint, which also carries the critic layout and the
index generator's state.

Not taken over from sac.hip: data-parallel training, the ring source inside the update (the batches are gathered by ONE
rlx_sac_replay_sample_f32 call in front of it), kept weight images, the full-jit networks and observation normalisation -- the
flags for them do not exist here."""
from rlx_amd.algorithms.redq.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.sac_ensemble import EnsembleSAC


def policy_lr(count, *, anneal, learning_rate, nr_envs, learning_starts, total_timesteps, q_update_steps=1):
    """policy_linear_schedule / entropy_linear_schedule (redq.py:88-98) at `count` previous policy steps"""
    if not anneal:
        return learning_rate
    return learning_rate * (1.0 - (count * nr_envs - learning_starts) / (total_timesteps - learning_starts))


def critic_lr_and_delta(count, *, anneal, learning_rate, nr_envs, learning_starts, total_timesteps, q_update_steps):
    """q_linear_schedule (redq.py:82-86) at `count` previous critic steps, and what one more step adds to it"""
    if not anneal:
        return learning_rate, 0.0
    span = (total_timesteps - learning_starts) * q_update_steps
    return learning_rate * (1.0 - (count * nr_envs - learning_starts) / span), -learning_rate * nr_envs / span


class REDQ(EnsembleSAC):
    """Also the base of aqe.hip and droq.hip, which share the high update-to-data loop: a subclass sets _NAME and _UPDATE (the
    context's update call) and overrides _read_ensemble (its hyper-parameters and refusals; critic_out_dim), hparams and
    critic_layout."""
    _NAME = "redq.hip"
    _COUNTERS = ("nr_q_updates", "nr_policy_updates")                  # BOTH optimizer step counts
    _UPDATE = "redq_update"

    def __init__(self, config, train_env, eval_env, run_path, writer):
        self._refuse(config.algorithm)
        self._read_ensemble(config.algorithm)
        super().__init__(config, train_env, eval_env, run_path, writer)
        self.nr_q_updates = 0                                          # redq.py:280; nr_policy_updates (:279) is SAC's opt_count
        self._init_critics(self.critic_out_dim)                        # critic.py:17-53, redq.py:115-116

    def _int_in(self, alg, name, lo, hi):
        v = int(getattr(alg, name))
        if not lo <= v <= hi:
            raise ValueError(f"{self._NAME}: {name} must be in {lo}..{hi}")
        return v

    def _read_ensemble(self, alg):
        self.ensemble_size = self._int_in(alg, "ensemble_size", 1, 16)
        self.in_target_minimization_size = int(alg.in_target_minimization_size)
        if not 1 <= self.in_target_minimization_size <= self.ensemble_size:
            raise ValueError(f"{self._NAME}: in_target_minimization_size must be in 1..ensemble_size")
        self.q_update_steps = self._int_in(alg, "q_update_steps", 1, 64)
        self.critic_out_dim = 1

    # the policy's / alpha's optimizer counter under SAC's name: SAC's loop, log line and schedule read it
    @property
    def opt_count(self):
        return self.nr_policy_updates

    @opt_count.setter
    def opt_count(self, v):
        self.nr_policy_updates = int(v)

    def _schedule_args(self):
        return dict(anneal=self.anneal_learning_rate, learning_rate=self.learning_rate, nr_envs=self.nr_envs,
                    learning_starts=self.learning_starts, total_timesteps=self.total_timesteps, q_update_steps=self.q_update_steps)

    def current_lr(self):
        return policy_lr(self.nr_policy_updates, **self._schedule_args())                                 # redq.py:88-92, :257

    def _common_hparams(self):
        """the fields the three hparams structs begin with: SAC's, the three learning rates (the critics' with its per-step delta,
        redq.py:82-98), Adam's"""
        lr = self.current_lr()
        lr_q, delta = critic_lr_and_delta(self.nr_q_updates, **self._schedule_args())
        return (self.gamma, self.tau, self.target_entropy, self.log_std_min, self.log_std_max, lr, lr_q, delta, lr, 0.9, 0.999, 1e-8)

    def hparams(self):
        from rlx_amd.hip import RedqHparams
        return RedqHparams(*self._common_hparams(), self.ensemble_size, self.in_target_minimization_size, self.q_update_steps)

    def _alloc(self):
        """SAC's buffers, with q_update_steps batches per update: [G * B, ...] = [G, B, ...] (replay_buffer.py:33-37)"""
        super()._alloc()
        t = self.torch
        n, O, A = self.q_update_steps * self.batch_size, self.obs_dim, self.act_dim
        f = dict(device=self.device, dtype=t.float32)
        self.batch = (t.zeros(n, O, **f), t.zeros(n, O, **f), t.zeros(n, A, **f), t.zeros(n, **f), t.zeros(n, **f))
        if self.obs_select:
            Op, Oc = self.policy_obs_dim, self.critic_obs_dim
            self.sel = (t.empty(n, Op, **f), t.empty(n, Op, **f), t.empty(n, Oc, **f), t.empty(n, Oc, **f))

    def update(self, batch):
        """One `update` (redq.py:144-261) on batch = (states, next_states, actions, rewards, terminations) of q_update_steps *
        batch_size rows, batch i in rows [i B, (i + 1) B): full observation rows, of which the policy's and the critics' columns
        are selected here when the env defines them."""
        hp = self.hparams()
        batch = self._select_columns(batch, hp)
        self.key, self.nr_q_updates, self.nr_policy_updates = getattr(self.ctx, self._UPDATE)(
            self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget,
            self.log_alpha, self.am, self.av, batch, self.key, self.nr_q_updates, self.nr_policy_updates, hp, self.metrics_dev, self.scheme)

    def sample_and_update(self):
        # replay_buffer.py:31-32: integers(size, B * G) then integers(nr_envs, B * G), one gather for all G batches
        self.idx1, self.idx2 = self._host_indices(self.batch_size * self.q_update_steps, self.nr_envs)
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch)

    def critic_layout(self):
        return {"ensemble_size": self.ensemble_size, "critic_params_per_net": int(self.nq), "critic_in_dim": int(self.qdesc.in_dim),
                "hidden": [self.nr_hidden_units, self.nr_hidden_units]}

    def _check_layout(self, layout):
        if layout != self.critic_layout():
            raise ValueError(f"{self._NAME}: the checkpoint's critic layout {layout} does not fit this configuration {self.critic_layout()}")

    def general_properties():
        return GeneralProperties
