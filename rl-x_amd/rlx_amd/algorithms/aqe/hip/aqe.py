"""aqe.hip -- AQE whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/aqe.hip).

The reference's AQE (rl_x/algorithms/aqe/flax/aqe.py) is its REDQ with another critic and target: every critic has
nr_heads_per_net outputs (critic.py), a critic step pools the values of ALL target networks, drops the nr_dropped_q_values largest
and takes the mean of the rest (aqe.py:164-165), and the policy ascends the mean over all heads (:197-200).  The host loop, acting,
the uniform warm-up, the replay ring, the sampling of q_update_steps batches at once, the two optimizer counters with their two
schedules (aqe.py:83-99 are redq.py:82-98) and the checkpoint are redq.hip's; this class derives from EnsembleSAC as REDQ does and
takes the schedules from the REDQ plugin.

Not taken over from sac.hip: what redq.hip leaves out (data-parallel training, the ring source inside the update, kept weight
images, the full-jit networks, observation normalisation)."""
from rlx_amd.algorithms.aqe.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.redq.hip.redq import critic_lr_and_delta, policy_lr
from rlx_amd.algorithms.sac_ensemble import EnsembleSAC


class AQE(EnsembleSAC):
    _NAME = "aqe.hip"
    _COUNTERS = ("nr_q_updates", "nr_policy_updates")                  # BOTH optimizer step counts

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        self._refuse(alg)
        self.ensemble_size = int(alg.ensemble_size)
        self.nr_heads_per_net = int(alg.nr_heads_per_net)
        self.nr_dropped_q_values = int(alg.nr_dropped_q_values)
        self.q_update_steps = int(alg.q_update_steps)
        if not 1 <= self.ensemble_size <= 16:
            raise ValueError("aqe.hip: ensemble_size must be in 1..16")
        if self.nr_heads_per_net < 1:
            raise ValueError("aqe.hip: nr_heads_per_net must be at least 1")
        self.nr_total_q_values = self.ensemble_size * self.nr_heads_per_net                               # aqe.py:58
        if self.nr_total_q_values > 128:
            raise ValueError("aqe.hip: ensemble_size * nr_heads_per_net (total q values) must be at most 128")
        if not 0 <= self.nr_dropped_q_values < self.nr_total_q_values:
            raise ValueError("aqe.hip: nr_dropped_q_values must be in 0..ensemble_size * nr_heads_per_net - 1")
        if not 1 <= self.q_update_steps <= 64:
            raise ValueError("aqe.hip: q_update_steps must be in 1..64")
        super().__init__(config, train_env, eval_env, run_path, writer)
        from rlx_amd.hip import AqeHparams
        self.AqeHparams = AqeHparams
        self.nr_q_updates = 0                                          # aqe.py:278; nr_policy_updates (:277) is SAC's opt_count
        self._init_critics(self.nr_heads_per_net)                      # critic.py, aqe.py:114-119

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
        return policy_lr(self.nr_policy_updates, **self._schedule_args())                                 # aqe.py:89-93, :255

    def hparams(self):
        lr = self.current_lr()
        lr_q, delta = critic_lr_and_delta(self.nr_q_updates, **self._schedule_args())
        return self.AqeHparams(self.gamma, self.tau, self.target_entropy, self.log_std_min, self.log_std_max, lr, lr_q, delta, lr, 0.9, 0.999,
                               1e-8, self.ensemble_size, self.nr_heads_per_net, self.nr_dropped_q_values, self.q_update_steps)

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
        """One `update` (aqe.py:145-259) on batch = (states, next_states, actions, rewards, terminations) of q_update_steps *
        batch_size rows, batch i in rows [i B, (i + 1) B): full observation rows, of which the policy's and the critics' columns
        are selected here when the env defines them."""
        hp = self.hparams()
        batch = self._select_columns(batch, hp)
        self.key, self.nr_q_updates, self.nr_policy_updates = self.ctx.aqe_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget,
            self.log_alpha, self.am, self.av, batch, self.key, self.nr_q_updates, self.nr_policy_updates, hp, self.metrics_dev, self.scheme)

    def sample_and_update(self):
        # replay_buffer.py:31-32: integers(size, B * G) then integers(nr_envs, B * G), one gather for all G batches
        self.idx1, self.idx2 = self._host_indices(self.batch_size * self.q_update_steps, self.nr_envs)
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch)

    def critic_layout(self):
        return {"ensemble_size": self.ensemble_size, "nr_heads_per_net": self.nr_heads_per_net, "critic_params_per_net": int(self.nq),
                "critic_in_dim": int(self.qdesc.in_dim), "hidden": [self.nr_hidden_units, self.nr_hidden_units]}

    def _check_layout(self, layout):
        if layout != self.critic_layout():
            raise ValueError(f"aqe.hip: the checkpoint's critic layout {layout} does not fit this configuration {self.critic_layout()}")

    def general_properties():
        return GeneralProperties
