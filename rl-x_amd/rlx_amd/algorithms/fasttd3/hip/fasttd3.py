"""`fasttd3.hip`: the FastTD3 training loop of rl_x/algorithms/fasttd3/pytorch/fasttd3.py:228-519 around the library's update
steps (rl-x_amd/csrc/fasttd3.hip).

Per vector step (fasttd3.py:260-282): act on the normalised observation (statistics frozen) with per-env exploration noise,
env.step on the processed action, ring add of the UNclipped action, noise scales redrawn where an episode ended.  Once
`learning_starts` steps are in the ring (:289): ONE sample of nr_policy_updates * nr_critic_updates * batch_size transitions
(:300), the observation normaliser updated on the sampled states and then on the next states (:301-302), and for every policy
update its critic updates -- each followed by the Polyak step, both inside rlx_fasttd3_critic_update_f32 -- and then the policy
step on the LAST critic slice's states (:312-324).

The replay ring, its sampling, the normaliser, the learning-rate schedule and evaluation are FastSAC's (the reference's two
algorithms share them: fasttd3/pytorch/replay_buffer.py, observation_normalizer.py); both plugins take them from
rlx_amd/algorithms/fast_offpolicy.py.  What differs from the reference, on purpose: random numbers (torch's CUDA generator
there; the library's counter RNG here, for the noise scales, the action noise and the replay indices alike), fp32 instead of bf16 autocast, parameters
initialised from numpy with torch.nn.Linear's defaults (uniform +-1/sqrt(fan_in); the policy head N(0, 0.01^2), bias 0,
policy.py:45,50-53)."""
import json
import logging
import os
import time

import numpy as np

from rlx_amd.algorithms.fast_offpolicy import FastOffPolicyLoop
from rlx_amd.algorithms.fasttd3.hip.general_properties import GeneralProperties
from rlx_amd.environments.data_interface_type import DataInterfaceType
from rlx_amd.plugin import MetricSink, adopt_checkpoint_config

rlx_logger = logging.getLogger("rl_x")

POLICY_HIDDEN = (512, 256, 128)      # policy.py:38-47
CRITIC_HIDDEN = (1024, 512, 256)     # q_network.py:28-36
CRITIC_METRICS = ("loss/q_loss", "q/q_min", "q/q_max", "gradients/critic_grad_norm")
POLICY_METRICS = ("loss/policy_loss", "gradients/policy_grad_norm")


def _torch_linear_flat(rng, in_dim, hidden, out_dim, head_std=None):
    """torch.nn.Linear's default initialisation in the flat layout (W[in, out], b per layer; then the head).  head_std: the
    policy head's layer_init (weights N(0, head_std^2), bias 0; policy.py:50-53)."""
    parts, d = [], in_dim
    for li, h in enumerate(list(hidden) + [out_dim]):
        bound = 1.0 / np.sqrt(d)
        if li == len(hidden) and head_std is not None:
            parts += [rng.normal(0.0, head_std, (d, h)), np.zeros(h)]
        else:
            parts += [rng.uniform(-bound, bound, (d, h)), rng.uniform(-bound, bound, h)]
        d = h
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


class FastTD3(FastOffPolicyLoop):
    _NAME = "fasttd3.hip"

    def __init__(self, config, train_env, eval_env, run_path, writer):
        import torch
        from rlx_amd.hip import Ctx, FastTd3Hparams, relu_mlp_desc
        from rlx_amd.hip import lib as hiplib
        self.torch, self.hiplib = torch, hiplib
        self.config, self.train_env, self.eval_env, self.writer = config, train_env, eval_env, writer
        alg = config.algorithm
        self.save_model = config.runner.save_model
        self.save_path = os.path.join(run_path, "models")
        self.seed = config.environment.seed
        self.nr_envs = int(config.environment.nr_envs)
        self.total_timesteps = int(alg.total_timesteps)
        self.learning_rate, self.anneal_learning_rate = float(alg.learning_rate), bool(alg.anneal_learning_rate)
        self.batch_size, self.capacity = int(alg.batch_size), int(alg.buffer_size_per_env)
        self.learning_starts, self.n_steps = int(alg.learning_starts), int(alg.n_steps)
        self.nr_critic_updates, self.nr_policy_updates = int(alg.nr_critic_updates_per_policy_update), int(alg.nr_policy_updates_per_step)
        self.logging_frequency, self.evaluation_frequency = int(alg.logging_frequency), int(alg.evaluation_frequency)
        self.save_frequency = int(alg.save_frequency)
        self.obs_norm = bool(alg.enable_observation_normalization)
        self.noise_std_min, self.noise_std_max = float(alg.noise_std_min), float(alg.noise_std_max)
        self.clip_and_rescale = bool(alg.action_clipping_and_rescaling)
        self.scheme = 1 if alg.threefry_partitionable else 0
        if self.logging_frequency % self.nr_envs != 0:                                        # fasttd3.py:62-63
            raise ValueError("The logging frequency must be a multiple of the number of environments.")
        if self.save_frequency != -1 and self.save_frequency % self.nr_envs != 0:             # fasttd3.py:65-66
            raise ValueError("The save frequency must be a multiple of the number of environments.")
        if alg.device != "gpu":
            raise ValueError("fasttd3.hip runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        if bool(alg.bf16_mixed_precision_training):
            raise ValueError("fasttd3.hip computes in fp32: set --algorithm.bf16_mixed_precision_training=False")
        if float(alg.max_grad_norm) != -1.0 and float(alg.max_grad_norm) <= 0.0:
            raise ValueError("fasttd3.hip: max_grad_norm must be -1 (off, the reference's sentinel) or positive")
        if train_env.general_properties.data_interface_type != DataInterfaceType.TORCH:
            raise ValueError("fasttd3.hip needs a TORCH data-interface environment")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("fasttd3.hip is single-GPU (its normaliser statistics and gradients are not all-reduced)")
        except ImportError:
            pass
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.ctx = Ctx(self.device.index or 0)
        self.sink = MetricSink(rlx_logger, writer, console=config.runner.track_console, tensorboard=config.runner.track_tb,
                               wandb=config.runner.track_wandb, rank=0)
        O = int(np.prod(train_env.single_observation_space.shape))
        A = int(np.prod(train_env.single_action_space.shape))
        self.obs_dim, self.act_dim = O, A
        from rlx_amd.algorithms.ppo.hip.ppo import PPO as _PPO
        pidx, cidx = _PPO._observation_indices(train_env, O)            # policy.py:13, q_network.py:11
        self.obs_select = pidx is not None
        self.policy_obs_dim, self.critic_obs_dim = (len(pidx), len(cidx)) if self.obs_select else (O, O)
        if self.obs_select:
            self.pidx, self.cidx = torch.from_numpy(pidx).to(self.device), torch.from_numpy(cidx).to(self.device)
        sp = train_env.single_action_space                              # policy.py:29-30
        self.act_low, self.act_high = (torch.from_numpy(np.asarray(getattr(sp, k), np.float32).reshape(-1).copy()).to(self.device)
                                       for k in ("low", "high"))
        self.pdesc = relu_mlp_desc(self.policy_obs_dim, POLICY_HIDDEN, A)
        self.qdesc = relu_mlp_desc(self.critic_obs_dim + A, CRITIC_HIDDEN, int(alg.nr_atoms))
        rng = np.random.default_rng(self.seed)
        self.pparams = torch.from_numpy(_torch_linear_flat(rng, self.policy_obs_dim, POLICY_HIDDEN, A, head_std=0.01)).to(self.device)
        q = np.concatenate([_torch_linear_flat(rng, self.critic_obs_dim + A, CRITIC_HIDDEN, int(alg.nr_atoms)) for _ in range(2)])
        self.qparams = torch.from_numpy(q).to(self.device)
        self.qtarget = self.qparams.clone()                             # critic.py:18-19
        z = torch.zeros_like
        self.pm, self.pv, self.qm, self.qv = z(self.pparams), z(self.pparams), z(self.qparams), z(self.qparams)
        self.critic_count = self.policy_count = 0
        self.key = hiplib.prng_key(self.seed)
        if self.obs_norm:     # observation_normalizer.py
            self.norm_mean, self.norm_var, self.norm_std = (torch.zeros(O, device=self.device), torch.ones(O, device=self.device),
                                                            torch.ones(O, device=self.device))
            self.norm_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.hp = FastTd3Hparams()
        for k in ("gamma", "tau", "v_min", "v_max", "weight_decay", "smoothing_epsilon", "smoothing_clip_value"):
            setattr(self.hp, k, float(alg[k]))
        self.hp.adam_b1, self.hp.adam_b2, self.hp.adam_eps = 0.9, 0.999, 1e-8       # torch.optim.AdamW defaults (fasttd3.py:88-89)
        self.hp.nr_atoms, self.hp.clipped_double_q = int(alg.nr_atoms), int(bool(alg.clipped_double_q_learning))
        self.hp.max_grad_norm = float(alg.max_grad_norm)
        self.horizon = getattr(train_env, "horizon", 1000)
        if self.save_model:
            os.makedirs(self.save_path, exist_ok=True)
            self.best_model_file_name = "latest.model"

    # ------------------------------------------------------------------ pieces
    def _alloc(self):
        """Training buffers: the replay ring, the sampled batch, the noise scales, metric accumulators."""
        t = self.torch
        N, O, A, cap = self.nr_envs, self.obs_dim, self.act_dim, self.capacity
        f = dict(device=self.device, dtype=t.float32)
        self.ring = (t.zeros(cap, N, O, **f), t.zeros(cap, N, O, **f), t.zeros(cap, N, A, **f), t.zeros(cap, N, **f), t.zeros(cap, N, **f),
                     t.zeros(cap, N, **f))                                # states, next_states, actions, rewards, dones, truncations
        self.pos = self.size = 0
        T = self.nr_policy_updates * self.nr_critic_updates * self.batch_size
        self.total = (t.empty(T, O, **f), t.empty(T, O, **f), t.empty(T, A, **f)) + tuple(t.empty(T, **f) for _ in range(4))
        self.idx_t, self.idx_e = t.empty(T, dtype=t.int32, device=self.device), t.empty(T, dtype=t.int32, device=self.device)
        if self.obs_select:
            Op, Oc = self.policy_obs_dim, self.critic_obs_dim
            self.sel = (t.empty(T, Op, **f), t.empty(T, Op, **f), t.empty(T, Oc, **f), t.empty(T, Oc, **f))
        self.noise_scales = t.empty(N, **f)
        self.metrics_c, self.metrics_p = t.zeros(4, **f), t.zeros(2, **f)
        # sums over the policy updates since the last log (the reference appends one metrics entry per policy update, each with
        # that block's last critic metrics, and averages them all: fasttd3.py:326-337)
        self.sum_c, self.sum_p, self.n_met = t.zeros(4, **f), t.zeros(2, **f), 0

    def _act_buffers(self, n):
        """(normalised obs, policy columns, action, processed action) for a batch of n envs"""
        bufs = self.__dict__.setdefault("_act_bufs", {})
        if n not in bufs:
            t = self.torch
            f = dict(device=self.device, dtype=t.float32)
            bufs[n] = (t.empty(n, self.obs_dim, **f), t.empty(n, self.policy_obs_dim, **f), t.empty(n, self.act_dim, **f),
                       t.empty(n, self.act_dim, **f))
        return bufs[n]

    def act_pair(self, state, deterministic=False):
        """normalize(update=False) + policy.get_action (fasttd3.py:262-264) -> (action for the ring, processed action for the env)"""
        act_norm, act_pobs, action, processed = self._act_buffers(int(state.shape[0]))
        x = self.normalize(state.contiguous(), act_norm, False)
        x = self._columns(x, self.pidx if self.obs_select else None, act_pobs)
        low, high = (self.act_low, self.act_high) if self.clip_and_rescale else (None, None)
        self.key = self.ctx.fasttd3_act(self.pdesc, self.pparams, x, None if deterministic else self.noise_scales, self.key, action,
                                        processed, deterministic=deterministic, low=low, high=high, scheme=self.scheme)
        return action, processed

    def act(self, state, deterministic=False):
        """the action the env gets (evaluation and test(): get_action(x) without noise)"""
        return self.act_pair(state, deterministic)[1]

    def redraw_noise_scales(self, dones=None):
        """noise scales for every env (dones None, fasttd3.py:241) or for the envs whose episode ended (:274-278)"""
        self.key = self.ctx.fasttd3_noise_scales(self.key, self.noise_scales, self.noise_std_min, self.noise_std_max, dones=dones,
                                                 scheme=self.scheme)

    def optimize(self, step_index):
        """fasttd3.py:296-341 for one vector step"""
        self.sample()
        s, s2 = self.total[0], self.total[1]
        self.normalize(s, s, True)                     # total_normalized_states (update=True), then the next states (:301-302)
        self.normalize(s2, s2, True)
        if self.obs_select:
            sp, s2p, sc, s2c = self.sel
            self.ctx.select_columns(s, self.pidx, sp)
            self.ctx.select_columns(s2, self.pidx, s2p)
            self.ctx.select_columns(s, self.cidx, sc)
            self.ctx.select_columns(s2, self.cidx, s2c)
        else:
            sp, s2p, sc, s2c = s, s2, None, None
        lr = self.current_lr(step_index)
        self.hp.lr_policy = self.hp.lr_critic = lr
        B = self.batch_size
        for i in range(self.nr_policy_updates):
            for j in range(self.nr_critic_updates):
                o = (i * self.nr_critic_updates + j) * B
                rows = slice(o, o + B)
                batch = (sp[rows], s2p[rows]) + tuple(x[rows] for x in self.total[2:])
                self.key, self.critic_count = self.ctx.fasttd3_critic_update(
                    self.pdesc, self.pparams, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget, batch, self.key, self.critic_count,
                    self.hp, self.metrics_c, self.scheme, critic_states=None if sc is None else sc[rows],
                    critic_next_states=None if s2c is None else s2c[rows])
            self.policy_count = self.ctx.fasttd3_policy_update(
                self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, sp[rows], self.policy_count, self.hp, self.metrics_p,
                critic_states=None if sc is None else sc[rows])
            self.sum_c += self.metrics_c            # one entry per policy update (device adds, no synchronisation)
            self.sum_p += self.metrics_p
            self.n_met += 1

    def _checked_means(self):
        """mean metrics since the last log as host lists (ONE device->host copy); raises on a non-finite value -- called before a
        checkpoint is written and before logging, so a poisoned state never replaces the last good file"""
        mc, mp = (self.sum_c / self.n_met).cpu().tolist(), (self.sum_p / self.n_met).cpu().tolist()
        if not all(np.isfinite(v) for v in mc + mp):
            raise FloatingPointError("fasttd3.hip: non-finite loss / gradient norm since the last log " + str(mc + mp) +
                                     " (the optimizer steps of the affected updates were skipped on the device; no checkpoint was "
                                     "written over the last good one)")
        return mc, mp

    # ------------------------------------------------------------------ training loop (fasttd3.py:228-446)
    def train(self):
        self._alloc()
        env = self.train_env
        state, _ = env.reset()
        state = state.clone()
        self.redraw_noise_scales()
        global_step = nr_episodes = opt_steps = 0
        last_log_time, last_log_step = time.time(), 0
        while global_step < self.total_timesteps:
            action, processed = self.act_pair(state)
            next_state, reward, terminated, truncated, info = env.step(processed)
            done = terminated | truncated
            donef = done.float()
            self.replay_add(state, next_state, action, reward, donef, truncated.float())          # fasttd3.py:272
            self.redraw_noise_scales(donef)                                                      # fasttd3.py:274-278
            state = next_state.clone()
            global_step += self.nr_envs
            if global_step > self.learning_starts * self.nr_envs:                                # fasttd3.py:289
                self.optimize(opt_steps)
                opt_steps += 1
            if self.evaluation_frequency != -1 and global_step % self.evaluation_frequency == 0:
                rets, lens = self.evaluate()
                self.last_eval = {"eval/episode_return": float(np.mean(rets)) if rets else float("nan"),
                                  "eval/episode_length": float(np.mean(lens)) if lens else float("nan")}
            if self.save_model and self.n_met and self.save_frequency != -1 and global_step % self.save_frequency == 0:
                self._checked_means()           # finite BEFORE the file is replaced
                self.save()
            if global_step % self.logging_frequency == 0 or global_step >= self.total_timesteps:
                now = time.time()
                combined = {}
                if self.n_met:
                    mc, mp = self._checked_means()                                              # one D2H per logging interval
                    combined.update(dict(zip(CRITIC_METRICS, mc)))
                    combined.update(dict(zip(POLICY_METRICS, mp)))
                if hasattr(env, "pop_episode_stats"):
                    n_done, mean_ret, mean_len = env.pop_episode_stats()
                    nr_episodes += n_done
                    if n_done:
                        combined.update({"rollout/episode_return": mean_ret, "rollout/episode_length": mean_len})
                combined.update(getattr(self, "last_eval", {}))
                combined.update({"steps/nr_env_steps": global_step, "steps/nr_critic_updates": self.critic_count,
                                 "steps/nr_policy_updates": self.policy_count, "steps/nr_episodes": nr_episodes,
                                 "lr/learning_rate": self.current_lr(opt_steps),
                                 "time/sps": int((global_step - last_log_step) / max(now - last_log_time, 1e-9))})
                last_log_time, last_log_step = now, global_step
                self.sum_c.zero_()
                self.sum_p.zero_()
                self.n_met = 0
                self.sink.write(global_step, combined)
                self.last_metrics = combined

    _STATE = ("pparams", "pm", "pv", "qparams", "qm", "qv", "qtarget")

    def save(self):
        """Native checkpoint: flat parameter / AdamW-moment vectors, normaliser statistics, counters, the algorithm config (the
        reference stores the modules' and optimisers' state_dicts, fasttd3.py:449-473)."""
        path = os.path.join(self.save_path, self.best_model_file_name)
        state = {k: getattr(self, k).cpu().numpy() for k in self._STATE + (self._NORM_STATE if self.obs_norm else ())}
        np.savez(path + ".tmp.npz", critic_count=self.critic_count, policy_count=self.policy_count, key=self.key,
                 config_algorithm=json.dumps(self.config.algorithm.to_dict()), **state)
        os.replace(path + ".tmp.npz", path)

    def load(config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)
        model = FastTD3(config, train_env, eval_env, run_path, writer)
        for k in FastTD3._STATE + (FastTD3._NORM_STATE if model.obs_norm else ()):
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        model.critic_count, model.policy_count = int(ckpt["critic_count"]), int(ckpt["policy_count"])
        model.key = ckpt["key"].astype(np.uint32)
        return model

    def general_properties():
        return GeneralProperties
