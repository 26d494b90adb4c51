"""droq.hip -- DroQ whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/droq.hip).

The reference's DroQ (rl_x/algorithms/droq/flax/droq.py) is its REDQ with dropout keys: the host loop, acting, warm-up, replay ring,
the sampling of q_update_steps batches at once, the two optimizer counters and their schedules are redq.py's line for line.  This
class therefore derives from `redq.hip`'s and imports its schedules.  What it replaces: the critics -- ensemble_size nets whose
hidden blocks are Dense -> Dropout -> LayerNorm -> ReLU (droq/flax/critic.py:25-35), flat and back to back, LayerNorm scale and bias
after every hidden bias -- the update call (rlx_droq_update_f32) and the critic layout a checkpoint carries, which also names the
LayerNorm and the dropout rate.

The dropout masks are the library's own documented stream from the reference's per-row dropout keys (include/rlx_hip.h, DESIGN.md
4.5g): flax folds hashed module paths into the dropout key, which cannot be restated."""
import numpy as np

from rlx_amd.algorithms.droq.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.redq.hip.redq import REDQ, critic_lr_and_delta, policy_lr  # noqa: F401  (the schedules are REDQ's)
from rlx_amd.algorithms.sac.hip.sac import _lecun_flat

MAX_HIDDEN = 768            # what the LayerNorm kernels hold in one wave (csrc/droq.hip)


def _with_layer_norm(flat, n_in, hidden, out_dim):
    """a plain flat net (W, b per layer) -> DroQ's layout: LayerNorm scale 1 and bias 0 after every hidden bias"""
    parts, off, d = [], 0, n_in
    for h in hidden:
        n = d * h + h
        parts += [flat[off:off + n], np.ones(h, np.float32), np.zeros(h, np.float32)]
        off, d = off + n, h
    parts.append(flat[off:])
    assert flat.size - off == d * out_dim + out_dim
    return np.concatenate(parts).astype(np.float32)


class DroQ(REDQ):
    _NAME = "droq.hip"
    _UPDATE = "droq_update"

    def _read_ensemble(self, alg):
        self.dropout_rate = float(alg.dropout_rate)
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("droq.hip: dropout_rate must be in [0, 1)")
        H = int(alg.nr_hidden_units)
        if H <= 0 or H % 64 != 0 or H > MAX_HIDDEN:
            raise ValueError(f"droq.hip: nr_hidden_units must be a multiple of 64, at most {MAX_HIDDEN} (the LayerNorm kernels' row width)")
        super()._read_ensemble(alg)
        if 3 * int(alg.batch_size) + 2 > 2 ** 31 - 1:
            raise ValueError("droq.hip: batch_size too large for the 32-bit key count 3 * batch_size + 2")

    def _init_critics(self, out_dim):
        """EnsembleSAC._init_critics (each net from its own split of critic_key, the target equal to the online critics, droq.py:64,
        :115-116), with flax's LayerNorm init -- scale 1, bias 0 -- in every hidden block (critic.py:29, :33)"""
        from rlx_amd.hip import ACT_RELU, mlp_desc
        torch = self.torch
        E, H, n_in = self.ensemble_size, self.nr_hidden_units, self.critic_obs_dim + self.act_dim
        self.qdesc = mlp_desc(n_in, [H, H], out_dim, ACT_RELU, False, False)
        critic_key = self.hiplib.threefry_split(self.hiplib.prng_key(self.seed), 4, self.scheme)[2]
        net_keys = self.hiplib.threefry_split(critic_key, E, self.scheme)
        q = np.concatenate([_with_layer_norm(_lecun_flat(np.random.default_rng([int(k[0]), int(k[1])]), n_in, [H, H], out_dim), n_in, [H, H],
                                             out_dim) for k in net_keys])
        self.nq = q.size // E
        self.qparams = torch.from_numpy(q).to(self.device)
        self.qtarget = self.qparams.clone()
        self.qm, self.qv = torch.zeros_like(self.qparams), torch.zeros_like(self.qparams)

    def hparams(self):
        from rlx_amd.hip import DroqHparams
        r = super().hparams()
        hp = DroqHparams()
        for name, _ in type(r)._fields_:
            setattr(hp, name, getattr(r, name))
        hp.dropout_rate = self.dropout_rate
        return hp

    def critic_layout(self):
        layout = super().critic_layout()
        layout.update(layer_norm=True, dropout_rate=self.dropout_rate)
        return layout

    def general_properties():
        return GeneralProperties
