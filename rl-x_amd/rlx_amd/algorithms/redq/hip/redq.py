"""redq.hip -- REDQ whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/redq.hip).

The reference's REDQ (rl_x/algorithms/redq/flax/redq.py) is its SAC host loop with an ensemble of scalar critics and a high
update-to-data `update`: policy.py is sac/flax's file, acting (redq.py:134-140), the uniform warm-up (:298-300) and the replay ring
are the same.  This class therefore derives from `sac.hip`'s and keeps its acting, warm-up actions, ring, `_host_indices`,
evaluation and `test`.  What it replaces: the critics -- ensemble_size independent nets with one output each (critic.py:17-53),
flat and back to back -- the sampling of q_update_steps batches at once (replay_buffer.py:30-38), the update call
(rlx_redq_update_f32: q_update_steps critic steps, then one policy / entropy step), the two optimizer counters with their two
schedules (redq.py:82-98) and the checkpoint, which also carries the critic layout and the index generator's state.

Not taken over from sac.hip: data-parallel training, the ring source inside the update (the batches are gathered by ONE
rlx_sac_replay_sample_f32 call in front of it), kept weight images, the full-jit networks and observation normalisation -- the
flags for them do not exist here."""
import json
import logging
import os

import numpy as np

from rlx_amd.algorithms.sac.hip.sac import SAC, _lecun_flat
from rlx_amd.algorithms.redq.hip.general_properties import GeneralProperties
from rlx_amd.plugin import adopt_checkpoint_config

rlx_logger = logging.getLogger("rl_x")


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


class REDQ(SAC):
    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        if alg.device != "gpu":
            raise ValueError("redq.hip runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("redq.hip is single-GPU (its gradients are not all-reduced)")
        except ImportError:
            pass
        if alg.get("network_architecture", "flax") != "flax":
            raise ValueError("redq.hip has the reference's flax networks only: algorithm.network_architecture must be 'flax'")
        if alg.get("enable_observation_normalization", False):
            raise ValueError("redq.hip has no observation normalisation (the reference's REDQ has none)")
        self.ensemble_size = int(alg.ensemble_size)
        self.in_target_minimization_size = int(alg.in_target_minimization_size)
        self.q_update_steps = int(alg.q_update_steps)
        if not 1 <= self.ensemble_size <= 16:
            raise ValueError("redq.hip: ensemble_size must be in 1..16")
        if not 1 <= self.in_target_minimization_size <= self.ensemble_size:
            raise ValueError("redq.hip: in_target_minimization_size must be in 1..ensemble_size")
        if not 1 <= self.q_update_steps <= 64:
            raise ValueError("redq.hip: q_update_steps must be in 1..64")
        super().__init__(config, train_env, eval_env, run_path, writer)
        torch = self.torch
        from rlx_amd.hip import ACT_RELU, RedqHparams, mlp_desc
        self.RedqHparams = RedqHparams
        self.keep_images = 0
        self.batch_states = True
        self.nr_q_updates = 0                                          # redq.py:280; nr_policy_updates (:279) is SAC's opt_count
        # critic.py:17-53: ensemble_size x (Dense(H) -> ReLU -> Dense(H) -> ReLU -> Dense(1)), each net from its own split of
        # critic_key; the target starts equal to the online critics (redq.py:115-116: both init(critic_key, ...))
        E, H, A = self.ensemble_size, self.nr_hidden_units, self.act_dim
        Oc = self.critic_obs_dim
        self.qdesc = mlp_desc(Oc + A, [H, H], 1, ACT_RELU, False, False)
        critic_key = self.hiplib.threefry_split(self.hiplib.prng_key(self.seed), 4, self.scheme)[2]       # redq.py:64
        net_keys = self.hiplib.threefry_split(critic_key, E, self.scheme)
        q = np.concatenate([_lecun_flat(np.random.default_rng([int(k[0]), int(k[1])]), Oc + A, [H, H], 1) for k in net_keys])
        self.nq = q.size // E
        self.qparams = torch.from_numpy(q).to(self.device)
        self.qtarget = self.qparams.clone()
        self.qm, self.qv = torch.zeros_like(self.qparams), torch.zeros_like(self.qparams)

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

    def hparams(self):
        lr = self.current_lr()
        lr_q, delta = critic_lr_and_delta(self.nr_q_updates, **self._schedule_args())
        return self.RedqHparams(self.gamma, self.tau, self.target_entropy, self.log_std_min, self.log_std_max, lr, lr_q, delta, lr, 0.9, 0.999,
                                1e-8, self.ensemble_size, self.in_target_minimization_size, self.q_update_steps)

    def parameters_written(self):
        """nothing is kept between calls: rlx_redq_update_f32 lays its weight images out per critic step"""

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
        if self.obs_select:
            sp, s2p, sc, s2c = self.sel
            self.ctx.select_columns(batch[0], self.pidx, sp)
            self.ctx.select_columns(batch[1], self.pidx, s2p)
            self.ctx.select_columns(batch[0], self.cidx, sc)
            self.ctx.select_columns(batch[1], self.cidx, s2c)
            batch = (sp, s2p) + tuple(batch[2:])
            hp.critic_states, hp.critic_next_states = sc.data_ptr(), s2c.data_ptr()
        self.key, self.nr_q_updates, self.nr_policy_updates = self.ctx.redq_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget,
            self.log_alpha, self.am, self.av, batch, self.key, self.nr_q_updates, self.nr_policy_updates, hp, self.metrics_dev, self.scheme)

    def sample_and_update(self):
        # replay_buffer.py:31-32: integers(size, B * G) then integers(nr_envs, B * G), one gather for all G batches
        self.idx1, self.idx2 = self._host_indices(self.batch_size * self.q_update_steps, self.nr_envs)
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch)

    _STATE = ("pparams", "pm", "pv", "qparams", "qm", "qv", "qtarget", "log_alpha", "am", "av")

    def critic_layout(self):
        return {"ensemble_size": self.ensemble_size, "critic_params_per_net": int(self.nq), "critic_in_dim": int(self.qdesc.in_dim),
                "hidden": [self.nr_hidden_units, self.nr_hidden_units]}

    def save(self):
        """Native checkpoint, one .npz: every parameter, moment and target vector, log_alpha, BOTH optimizer step counts, the key,
        the index generator's state, the critic layout and the algorithm config (the reference zips an orbax PyTree +
        config_algorithm.json, redq.py:458-473)."""
        os.makedirs(self.save_path, exist_ok=True)
        path = os.path.join(self.save_path, getattr(self, "best_model_file_name", "best.model"))
        state = {k: getattr(self, k).cpu().numpy() for k in self._STATE}
        np.savez(path + ".tmp.npz", nr_q_updates=self.nr_q_updates, nr_policy_updates=self.nr_policy_updates, key=self.key,
                 critic_layout=json.dumps(self.critic_layout()), rng_state=json.dumps(self.consumed_rng_state()),
                 config_algorithm=json.dumps(self.config.algorithm.to_dict()), **state)
        os.replace(path + ".tmp.npz", path)
        return path

    def load(config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)   # redq.py:483-486
        model = REDQ(config, train_env, eval_env, run_path, writer)
        layout = json.loads(str(ckpt["critic_layout"]))
        if layout != model.critic_layout():
            raise ValueError(f"redq.hip: the checkpoint's critic layout {layout} does not fit this configuration {model.critic_layout()}")
        for k in REDQ._STATE:
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        model.nr_q_updates = int(ckpt["nr_q_updates"])
        model.nr_policy_updates = int(ckpt["nr_policy_updates"])
        model.key = ckpt["key"].astype(np.uint32)
        model.rng.bit_generator.state = json.loads(str(ckpt["rng_state"]))
        return model

    def general_properties():
        return GeneralProperties
