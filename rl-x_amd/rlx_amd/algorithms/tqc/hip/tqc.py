"""tqc.hip -- TQC whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/tqc.hip).

The reference's TQC (rl_x/algorithms/tqc/flax/tqc.py) is its SAC host loop with another critic: policy.py and replay_buffer.py
are sac/flax's files, acting (tqc.py:126-131), the uniform warm-up (:266-268), the replay ring, the host index draws and the key
schedule (:67, :211-212) are the same.  This class therefore derives from `sac.hip`'s and keeps its acting, warm-up actions, ring,
`_host_indices`, evaluation and `test`.  What it replaces: the critics -- ensemble_size independent nets with nr_atoms_per_net
outputs each (critic.py:17-55), flat and back to back -- the update call (rlx_tqc_update_f32) and the checkpoint, which also
carries the critic layout and the index generator's state.

Not taken over from sac.hip: data-parallel training, the ring source inside the update (the batch is gathered by
rlx_sac_replay_sample_f32 in front of it), kept weight images, the full-jit networks and observation normalisation -- the flags
for them do not exist here."""
import json
import logging
import os

import numpy as np

from rlx_amd.algorithms.sac.hip.sac import SAC, _lecun_flat
from rlx_amd.algorithms.tqc.hip.general_properties import GeneralProperties
from rlx_amd.plugin import adopt_checkpoint_config

rlx_logger = logging.getLogger("rl_x")


class TQC(SAC):
    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        if alg.device != "gpu":
            raise ValueError("tqc.hip runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("tqc.hip is single-GPU (its gradients are not all-reduced)")
        except ImportError:
            pass
        if alg.get("network_architecture", "flax") != "flax":
            raise ValueError("tqc.hip has the reference's flax networks only: algorithm.network_architecture must be 'flax'")
        if alg.get("enable_observation_normalization", False):
            raise ValueError("tqc.hip has no observation normalisation (the reference's TQC has none)")
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
        torch = self.torch
        from rlx_amd.hip import ACT_RELU, TqcHparams, mlp_desc
        self.TqcHparams = TqcHparams
        self.keep_images = 0
        self.batch_states = True
        # critic.py:17-55: ensemble_size x (Dense(H) -> ReLU -> Dense(H) -> ReLU -> Dense(nr_atoms_per_net)), each net from its own
        # split of critic_key; the target starts equal to the online critics (tqc.py:106-107: both init(critic_key, ...))
        E, N, H, A = self.ensemble_size, self.nr_atoms_per_net, self.nr_hidden_units, self.act_dim
        Oc = self.critic_obs_dim
        self.qdesc = mlp_desc(Oc + A, [H, H], N, ACT_RELU, False, False)
        critic_key = self.hiplib.threefry_split(self.hiplib.prng_key(self.seed), 4, self.scheme)[2]       # tqc.py:67
        net_keys = self.hiplib.threefry_split(critic_key, E, self.scheme)
        q = np.concatenate([_lecun_flat(np.random.default_rng([int(k[0]), int(k[1])]), Oc + A, [H, H], N) for k in net_keys])
        self.nq = q.size // E
        self.qparams = torch.from_numpy(q).to(self.device)
        self.qtarget = self.qparams.clone()
        self.qm, self.qv = torch.zeros_like(self.qparams), torch.zeros_like(self.qparams)

    def hparams(self):
        lr = self.current_lr()                                          # tqc.py:85-93: one schedule for the three optimisers
        hp = self.TqcHparams(self.gamma, self.tau, self.target_entropy, self.log_std_min, self.log_std_max, lr, lr, lr, 0.9, 0.999, 1e-8,
                             self.huber_kappa, self.ensemble_size, self.nr_atoms_per_net, self.nr_dropped_atoms_per_net)
        return hp

    def parameters_written(self):
        """nothing is kept between calls: rlx_tqc_update_f32 lays its weight images out per call"""

    def update(self, batch):
        """One `update` (tqc.py:134-230) on batch = (states, next_states, actions, rewards, terminations): full observation rows,
        of which the policy's and the critics' columns are selected here when the env defines them."""
        hp = self.hparams()
        if self.obs_select:
            sp, s2p, sc, s2c = self.sel
            self.ctx.select_columns(batch[0], self.pidx, sp)
            self.ctx.select_columns(batch[1], self.pidx, s2p)
            self.ctx.select_columns(batch[0], self.cidx, sc)
            self.ctx.select_columns(batch[1], self.cidx, s2c)
            batch = (sp, s2p) + tuple(batch[2:])
            hp.critic_states, hp.critic_next_states = sc.data_ptr(), s2c.data_ptr()
        self.key, self.opt_count = self.ctx.tqc_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget,
            self.log_alpha, self.am, self.av, batch, self.key, self.opt_count, hp, self.metrics_dev, self.scheme)

    def sample_and_update(self):
        self.idx1, self.idx2 = self._host_indices(self.batch_size, self.nr_envs)      # replay_buffer.py:31-32
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch)

    _STATE = ("pparams", "pm", "pv", "qparams", "qm", "qv", "qtarget", "log_alpha", "am", "av")

    def save(self):
        """Native checkpoint, one .npz: every parameter, moment and target vector, log_alpha, the optimizer step count, the key,
        the index generator's state, the critic layout and the algorithm config (the reference zips an orbax PyTree +
        config_algorithm.json, tqc.py:423-438)."""
        os.makedirs(self.save_path, exist_ok=True)
        path = os.path.join(self.save_path, getattr(self, "best_model_file_name", "best.model"))
        state = {k: getattr(self, k).cpu().numpy() for k in self._STATE}
        layout = {"ensemble_size": self.ensemble_size, "nr_atoms_per_net": self.nr_atoms_per_net, "critic_params_per_net": int(self.nq),
                  "critic_in_dim": int(self.qdesc.in_dim), "hidden": [self.nr_hidden_units, self.nr_hidden_units]}
        np.savez(path + ".tmp.npz", opt_count=self.opt_count, key=self.key, critic_layout=json.dumps(layout),
                 rng_state=json.dumps(self.consumed_rng_state()), config_algorithm=json.dumps(self.config.algorithm.to_dict()), **state)
        os.replace(path + ".tmp.npz", path)
        return path

    def load(config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)   # tqc.py:448-451
        model = TQC(config, train_env, eval_env, run_path, writer)
        layout = json.loads(str(ckpt["critic_layout"]))
        if (layout["ensemble_size"], layout["nr_atoms_per_net"], layout["critic_params_per_net"]) != (
                model.ensemble_size, model.nr_atoms_per_net, int(model.nq)):
            raise ValueError(f"tqc.hip: the checkpoint's critic layout {layout} does not fit this configuration")
        for k in TQC._STATE:
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        model.opt_count = int(ckpt["opt_count"])
        model.key = ckpt["key"].astype(np.uint32)
        model.rng.bit_generator.state = json.loads(str(ckpt["rng_state"]))
        return model

    def general_properties():
        return GeneralProperties
