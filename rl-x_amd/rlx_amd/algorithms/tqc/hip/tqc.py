"""tqc.hip -- TQC whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/tqc.hip).

The reference's TQC (rl_x/algorithms/tqc/flax/tqc.py) is its SAC host loop with another critic: policy.py and replay_buffer.py
are sac/flax's files, acting (tqc.py:126-131), the uniform warm-up (:266-268), the replay ring, the host index draws and the key
schedule (:67, :211-212) are the same.  This class therefore derives from `sac.hip`'s (through EnsembleSAC, what it shares with
redq.hip) and keeps its acting, warm-up actions, ring, `_host_indices`, evaluation and `test`.  What it replaces: the critics --
ensemble_size independent nets with nr_atoms_per_net outputs each (critic.py:17-55), flat and back to back -- the update call
(rlx_tqc_update_f32) and the checkpoint, which also carries the critic layout and the index generator's state.

Not taken over from sac.hip: data-parallel training, the ring source inside the update (the batch is gathered by
rlx_sac_replay_sample_f32 in front of it), kept weight images, the full-jit networks and observation normalisation -- the flags
for them do not exist here."""
from rlx_amd.algorithms.sac_ensemble import EnsembleSAC
from rlx_amd.algorithms.tqc.hip.general_properties import GeneralProperties


class TQC(EnsembleSAC):
    _NAME = "tqc.hip"
    _COUNTERS = ("opt_count",)

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        self._refuse(alg)
        self.ensemble_size = int(alg.ensemble_size)
        self.nr_atoms_per_net = int(alg.nr_atoms_per_net)
        self.nr_dropped_atoms_per_net = int(alg.nr_dropped_atoms_per_net)
        self.huber_kappa = float(alg.huber_kappa)
        self.nr_total_atoms = self.nr_atoms_per_net * self.ensemble_size                                  # tqc.py:60
        self.nr_target_atoms = self.nr_total_atoms - self.nr_dropped_atoms_per_net * self.ensemble_size   # tqc.py:61
        if not 1 <= self.ensemble_size <= 8:
            raise ValueError("tqc.hip: ensemble_size must be in 1..8")
        if self.nr_atoms_per_net < 1 or self.nr_total_atoms > 128:
            raise ValueError("tqc.hip: nr_atoms_per_net must be at least 1 and ensemble_size * nr_atoms_per_net at most 128")
        if not 0 <= self.nr_dropped_atoms_per_net < self.nr_atoms_per_net:
            raise ValueError("tqc.hip: nr_dropped_atoms_per_net must be in [0, nr_atoms_per_net)")
        if not self.huber_kappa > 0:
            raise ValueError("tqc.hip: huber_kappa must be positive")
        super().__init__(config, train_env, eval_env, run_path, writer)
        from rlx_amd.hip import TqcHparams
        self.TqcHparams = TqcHparams
        self._init_critics(self.nr_atoms_per_net)                      # critic.py:17-55, tqc.py:106-107

    def hparams(self):
        lr = self.current_lr()                                          # tqc.py:85-93: one schedule for the three optimisers
        hp = self.TqcHparams(self.gamma, self.tau, self.target_entropy, self.log_std_min, self.log_std_max, lr, lr, lr, 0.9, 0.999, 1e-8,
                             self.huber_kappa, self.ensemble_size, self.nr_atoms_per_net, self.nr_dropped_atoms_per_net)
        return hp

    def update(self, batch):
        """One `update` (tqc.py:134-230) on batch = (states, next_states, actions, rewards, terminations): full observation rows,
        of which the policy's and the critics' columns are selected here when the env defines them."""
        hp = self.hparams()
        batch = self._select_columns(batch, hp)
        self.key, self.opt_count = self.ctx.tqc_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget,
            self.log_alpha, self.am, self.av, batch, self.key, self.opt_count, hp, self.metrics_dev, self.scheme)

    def sample_and_update(self):
        self.idx1, self.idx2 = self._host_indices(self.batch_size, self.nr_envs)      # replay_buffer.py:31-32
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch)

    def critic_layout(self):
        return {"ensemble_size": self.ensemble_size, "nr_atoms_per_net": self.nr_atoms_per_net, "critic_params_per_net": int(self.nq),
                "critic_in_dim": int(self.qdesc.in_dim), "hidden": [self.nr_hidden_units, self.nr_hidden_units]}

    def _check_layout(self, layout):
        if (layout["ensemble_size"], layout["nr_atoms_per_net"], layout["critic_params_per_net"]) != (
                self.ensemble_size, self.nr_atoms_per_net, int(self.nq)):
            raise ValueError(f"tqc.hip: the checkpoint's critic layout {layout} does not fit this configuration")

    def general_properties():
        return GeneralProperties
