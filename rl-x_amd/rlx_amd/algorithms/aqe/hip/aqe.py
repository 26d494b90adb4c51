"""aqe.hip -- AQE whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/aqe.hip).

The reference's AQE (rl_x/algorithms/aqe/flax/aqe.py) is its REDQ with another critic and target: every critic has
nr_heads_per_net outputs (critic.py), a critic step pools the values of ALL target networks, drops the nr_dropped_q_values largest
and takes the mean of the rest (aqe.py:164-165), and the policy ascends the mean over all heads (:197-200).  The host loop, acting,
the uniform warm-up, the replay ring, the sampling of q_update_steps batches at once, the two optimizer counters with their two
schedules (aqe.py:83-99 are redq.py:82-98) and the checkpoint are redq.hip's: this class derives from the REDQ plugin's and keeps
its own hyper-parameters and refusals, hparams struct, head width, critic layout and update call.

Not taken over from sac.hip: what redq.hip leaves out (data-parallel training, the ring source inside the update, kept weight
images, the full-jit networks, observation normalisation)."""
from rlx_amd.algorithms.aqe.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.redq.hip.redq import REDQ, critic_lr_and_delta, policy_lr  # noqa: F401  (the schedules are REDQ's)


class AQE(REDQ):
    _NAME = "aqe.hip"
    _UPDATE = "aqe_update"

    def _read_ensemble(self, alg):
        self.ensemble_size = self._int_in(alg, "ensemble_size", 1, 16)
        self.nr_heads_per_net = int(alg.nr_heads_per_net)
        self.nr_dropped_q_values = int(alg.nr_dropped_q_values)
        if self.nr_heads_per_net < 1:
            raise ValueError("aqe.hip: nr_heads_per_net must be at least 1")
        self.nr_total_q_values = self.ensemble_size * self.nr_heads_per_net                               # aqe.py:58
        if self.nr_total_q_values > 128:
            raise ValueError("aqe.hip: ensemble_size * nr_heads_per_net (total q values) must be at most 128")
        if not 0 <= self.nr_dropped_q_values < self.nr_total_q_values:
            raise ValueError("aqe.hip: nr_dropped_q_values must be in 0..ensemble_size * nr_heads_per_net - 1")
        self.q_update_steps = self._int_in(alg, "q_update_steps", 1, 64)
        self.critic_out_dim = self.nr_heads_per_net                    # critic.py, aqe.py:114-119

    def hparams(self):
        from rlx_amd.hip import AqeHparams
        return AqeHparams(*self._common_hparams(), self.ensemble_size, self.nr_heads_per_net, self.nr_dropped_q_values, self.q_update_steps)

    def critic_layout(self):
        return {"ensemble_size": self.ensemble_size, "nr_heads_per_net": self.nr_heads_per_net, "critic_params_per_net": int(self.nq),
                "critic_in_dim": int(self.qdesc.in_dim), "hidden": [self.nr_hidden_units, self.nr_hidden_units]}

    def general_properties():
        return GeneralProperties
