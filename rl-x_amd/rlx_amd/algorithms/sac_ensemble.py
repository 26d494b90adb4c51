"""The pieces tqc.hip and redq.hip (with it aqe.hip and droq.hip, its subclasses) share: all are sac.hip's host loop with an ensemble of independent ReLU critics, flat and back
to back, whose update takes gathered batches (csrc/sac_ens.h is the same layer on the library's side).

A subclass is named as the reference's algorithm is and sets the class attributes _NAME (the plugin's name) and _COUNTERS (the
optimizer step counts a checkpoint carries, by attribute name).  Its __init__ calls _refuse(config.algorithm), validates its own
hyper-parameters, then super().__init__(...), then _init_critics(out_dim).  It provides hparams(), update(batch) -- which passes
its batch through _select_columns(batch, hp) -- sample_and_update(), critic_layout() -> the dict a checkpoint stores, and
_check_layout(layout), which raises ValueError when a loaded layout does not fit this configuration."""
import json
import os

import numpy as np

from rlx_amd.algorithms.sac.hip.sac import SAC, _lecun_flat
from rlx_amd.plugin import adopt_checkpoint_config


class EnsembleSAC(SAC):
    _NAME = None
    _COUNTERS = ()

    def _refuse(self, alg):
        """what sac.hip offers and these plugins do not: raised in front of anything that touches a device"""
        if alg.device != "gpu":
            raise ValueError(f"{self._NAME} runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError(f"{self._NAME} is single-GPU (its gradients are not all-reduced)")
        except ImportError:
            pass
        if alg.get("network_architecture", "flax") != "flax":
            raise ValueError(f"{self._NAME} has the reference's flax networks only: algorithm.network_architecture must be 'flax'")
        if alg.get("enable_observation_normalization", False):
            raise ValueError(f"{self._NAME} has no observation normalisation (the reference's {type(self).__name__} has none)")

    def __init__(self, config, train_env, eval_env, run_path, writer):
        super().__init__(config, train_env, eval_env, run_path, writer)
        self.keep_images = 0
        self.batch_states = True

    def _init_critics(self, out_dim):
        """critic.py: ensemble_size x (Dense(H) -> ReLU -> Dense(H) -> ReLU -> Dense(out_dim)), each net from its own split of
        critic_key (tqc.py:67, redq.py:64); the target starts equal to the online critics (both init(critic_key, ...))"""
        from rlx_amd.hip import ACT_RELU, mlp_desc
        torch = self.torch
        E, H, n_in = self.ensemble_size, self.nr_hidden_units, self.critic_obs_dim + self.act_dim
        self.qdesc = mlp_desc(n_in, [H, H], out_dim, ACT_RELU, False, False)
        critic_key = self.hiplib.threefry_split(self.hiplib.prng_key(self.seed), 4, self.scheme)[2]
        net_keys = self.hiplib.threefry_split(critic_key, E, self.scheme)
        q = np.concatenate([_lecun_flat(np.random.default_rng([int(k[0]), int(k[1])]), n_in, [H, H], out_dim) for k in net_keys])
        self.nq = q.size // E
        self.qparams = torch.from_numpy(q).to(self.device)
        self.qtarget = self.qparams.clone()
        self.qm, self.qv = torch.zeros_like(self.qparams), torch.zeros_like(self.qparams)

    def parameters_written(self):
        """nothing is kept between calls: the update lays its weight images out per call (REDQ: per critic step)"""

    def _select_columns(self, batch, hp):
        """batch holds full observation rows: when the env defines the policy's and the critics' columns, select them (the
        critics' go to hp.critic_states / critic_next_states)"""
        if not self.obs_select:
            return batch
        sp, s2p, sc, s2c = self.sel
        self.ctx.select_columns(batch[0], self.pidx, sp)
        self.ctx.select_columns(batch[1], self.pidx, s2p)
        self.ctx.select_columns(batch[0], self.cidx, sc)
        self.ctx.select_columns(batch[1], self.cidx, s2c)
        hp.critic_states, hp.critic_next_states = sc.data_ptr(), s2c.data_ptr()
        return (sp, s2p) + tuple(batch[2:])

    _STATE = ("pparams", "pm", "pv", "qparams", "qm", "qv", "qtarget", "log_alpha", "am", "av")

    def save(self):
        """Native checkpoint, one .npz: every parameter, moment and target vector, log_alpha, the optimizer step counts
        (_COUNTERS), the key, the index generator's state, the critic layout and the algorithm config (the reference zips an orbax
        PyTree + config_algorithm.json, tqc.py:423-438, redq.py:458-473)."""
        os.makedirs(self.save_path, exist_ok=True)
        path = os.path.join(self.save_path, getattr(self, "best_model_file_name", "best.model"))
        state = {k: getattr(self, k).cpu().numpy() for k in self._STATE}
        counters = {k: getattr(self, k) for k in self._COUNTERS}
        np.savez(path + ".tmp.npz", **counters, key=self.key, critic_layout=json.dumps(self.critic_layout()),
                 rng_state=json.dumps(self.consumed_rng_state()), config_algorithm=json.dumps(self.config.algorithm.to_dict()), **state)
        os.replace(path + ".tmp.npz", path)
        return path

    @classmethod
    def load(cls, config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)   # tqc.py:448-451
        model = cls(config, train_env, eval_env, run_path, writer)
        model._check_layout(json.loads(str(ckpt["critic_layout"])))
        for k in cls._STATE:
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        for k in cls._COUNTERS:
            setattr(model, k, int(ckpt[k]))
        model.key = ckpt["key"].astype(np.uint32)
        model.rng.bit_generator.state = json.loads(str(ckpt["rng_state"]))
        return model
