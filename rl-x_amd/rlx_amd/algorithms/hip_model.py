"""The host layer of a plugin that drives the HIP library: fastsac.hip, fasttd3.hip, mpo.hip and fastmpo.hip (through
rlx_amd/algorithms/fast_offpolicy.py) and reppo.hip build on `HipModel`.

A subclass's __init__ runs the set-up in two steps around its own flags and validations:

    alg = self._read_flags(config, train_env, eval_env, run_path, writer)   # no torch, no device: flags and the common refusals
    ...                                                                      # the plugin's own flags and refusals
    self._open_device()                                                      # torch, device, ctx, sink, dimensions, index sets, key

so that everything that can be refused without a device is refused before torch is imported and before a Ctx is opened.  The
class attributes _NAME (the plugin's name), _FILE, _STATE and _COUNTERS describe its checkpoint."""
import json
import logging
import os
import time

import numpy as np

from rlx_amd.environments.data_interface_type import DataInterfaceType
from rlx_amd.plugin import MetricSink, adopt_checkpoint_config

rlx_logger = logging.getLogger("rl_x")

TRUNC_NORMAL_STD = 0.87962566103423978               # std of a unit normal truncated at +-2 (jax.nn.initializers.variance_scaling)


def observation_indices(env, obs_dim):
    """(policy columns, critic columns) as int32 arrays when the env defines either index set, else (None, None).
    A missing set means all columns (`getattr(env, ..., jnp.arange(obs_dim))`, ppo/flax/policy.py:13)."""
    pidx = getattr(env, "policy_observation_indices", None)
    cidx = getattr(env, "critic_observation_indices", None)
    if pidx is None and cidx is None:
        return None, None
    out = []
    for name, idx in (("policy", pidx), ("critic", cidx)):
        idx = np.arange(obs_dim) if idx is None else np.asarray(idx).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= obs_dim:
            raise ValueError(f"{name}_observation_indices must be non-empty and within [0, {obs_dim})")
        out.append(np.ascontiguousarray(idx, dtype=np.int32))
    return out[0], out[1]


def torch_linear_flat(rng, in_dim, hidden, out_dim, layer_norm, head_std=None):
    """torch.nn.Linear's default initialisation (uniform +-1/sqrt(fan_in)) in the library's flat layout: W[in, out], b and, with
    layer_norm, LayerNorm scale 1 / bias 0 per hidden layer; then the head.  head_std: None for the default head, 0 for a zero
    head (FastSAC's policy, policy.py:58-59), else weights N(0, head_std^2) and bias 0 (FastTD3's layer_init, policy.py:50-53)."""
    parts, d = [], in_dim
    for h in hidden:
        bound = 1.0 / np.sqrt(d)
        parts += [rng.uniform(-bound, bound, (d, h)), rng.uniform(-bound, bound, h)]
        if layer_norm:
            parts += [np.ones(h), np.zeros(h)]
        d = h
    if head_std is None:
        bound = 1.0 / np.sqrt(d)
        parts += [rng.uniform(-bound, bound, (d, out_dim)), rng.uniform(-bound, bound, out_dim)]
    else:
        parts += [rng.normal(0.0, head_std, (d, out_dim)) if head_std else np.zeros((d, out_dim)), np.zeros(out_dim)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def eval_means(rets, lens):
    return {"eval/episode_return": float(np.mean(rets)) if rets else float("nan"),
            "eval/episode_length": float(np.mean(lens)) if lens else float("nan")}


class HipModel:
    _NAME = None
    _FILE = "latest.model"          # the checkpoint's file name under save_path
    _STATE = ()                     # device tensors a checkpoint holds
    _NORM_STATE = ("norm_mean", "norm_var", "norm_std", "norm_count")       # ... and these when obs_norm
    _COUNTERS = ()                  # host integers (or tuples of them) a checkpoint holds

    # ------------------------------------------------------------------ set-up
    def _read_flags(self, config, train_env, eval_env, run_path, writer):
        """Step one: the flags every plugin has and the refusals that need neither torch nor a device -> config.algorithm"""
        alg = config.algorithm
        if alg.device != "gpu":
            raise ValueError(self._NAME + " runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        if bool(alg.get("bf16_mixed_precision_training", False)):
            raise ValueError(self._NAME + " computes in fp32: set --algorithm.bf16_mixed_precision_training=False")
        self.config, self.train_env, self.eval_env, self.writer = config, train_env, eval_env, writer
        self.save_model = config.runner.save_model
        self.save_path = os.path.join(run_path, "models")
        self.seed = config.environment.seed
        self.nr_envs = int(config.environment.nr_envs)
        self.total_timesteps = int(alg.total_timesteps)
        self.scheme = 1 if alg.threefry_partitionable else 0
        return alg

    def _open_device(self, torch_env_only=True):
        """Step two: the refusals that need the env or torch, then torch, device, ctx, sink, the env's dimensions and observation
        index sets, horizon, key and the save directory"""
        env = self.train_env
        if torch_env_only and env.general_properties.data_interface_type != DataInterfaceType.TORCH:
            raise ValueError(self._NAME + " needs a TORCH data-interface environment")
        import torch
        from rlx_amd.hip import Ctx
        from rlx_amd.hip import lib as hiplib
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError(self._NAME + " is single-GPU (its normaliser statistics and gradients are not all-reduced)")
        except ImportError:
            pass
        self.torch, self.hiplib = torch, hiplib
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.ctx = Ctx(self.device.index or 0)
        config = self.config
        self.sink = MetricSink(rlx_logger, self.writer, console=config.runner.track_console, tensorboard=config.runner.track_tb,
                               wandb=config.runner.track_wandb, rank=0)
        O = int(np.prod(env.single_observation_space.shape))
        self.obs_dim, self.act_dim = O, int(np.prod(env.single_action_space.shape))
        pidx, cidx = observation_indices(env, O)
        self.obs_select = pidx is not None
        self.policy_obs_dim, self.critic_obs_dim = (len(pidx), len(cidx)) if self.obs_select else (O, O)
        self.pidx = torch.from_numpy(pidx).to(self.device) if self.obs_select else None
        self.cidx = torch.from_numpy(cidx).to(self.device) if self.obs_select else None
        self.horizon = getattr(env, "horizon", 1000)
        self.key = hiplib.prng_key(self.seed)
        if self.save_model:
            os.makedirs(self.save_path, exist_ok=True)

    def _alloc_normalizer(self):
        """ObservationNormalizer's statistics (observation_normalizer.py:19-23): mean 0, var 1, std 1, an int64 count"""
        if self.obs_norm:
            t, O = self.torch, self.obs_dim
            self.norm_mean, self.norm_var, self.norm_std = (t.zeros(O, device=self.device), t.ones(O, device=self.device),
                                                            t.ones(O, device=self.device))
            self.norm_count = t.zeros(1, dtype=t.int64, device=self.device)

    def _action_bounds(self):
        """The action space's operands on the device: act_low, act_high and action_scale = max(|low - center|, |high - center|) /
        scale (fastsac policy.py:36-43); spaces without center / scale: mid-point, 1 -> (low, high) on the host"""
        sp = self.train_env.single_action_space
        low, high = (np.asarray(getattr(sp, k), np.float32).reshape(-1) for k in ("low", "high"))
        center = np.asarray(getattr(sp, "center", 0.5 * (low + high)), np.float32).reshape(-1)
        scale = np.asarray(getattr(sp, "scale", np.ones(self.act_dim)), np.float32).reshape(-1)
        t = lambda a: self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
        self.act_low, self.act_high = t(low.copy()), t(high.copy())
        self.action_scale = t(np.maximum(np.abs(low - center), np.abs(high - center)) / scale)
        return low, high

    def _act_buffers(self, n):
        """(normalised obs, action, processed action) for a batch of n envs -- the eval env may have another nr_envs than the
        train env; test() / evaluate() need only these"""
        bufs = self.__dict__.setdefault("_act_bufs", {})
        if n not in bufs:
            t, f = self.torch, dict(device=self.device, dtype=self.torch.float32)
            bufs[n] = (t.empty(n, self.obs_dim, **f), t.empty(n, self.act_dim, **f), t.empty(n, self.act_dim, **f))
        return bufs[n]

    # ------------------------------------------------------------------ logging
    def _finite(self, values, when="since the last log", note=""):
        if not all(np.isfinite(v) for v in values):
            raise FloatingPointError(f"{self._NAME}: non-finite loss / gradient norm {when} {values}{note}")
        return values

    def _mean_metrics(self, *sums, note=""):
        """mean of the metric sums over the n_met updates since the last log as one host list (one device->host copy per sum);
        raises on a non-finite value"""
        return self._finite([v for s in sums for v in (s / self.n_met).cpu().tolist()], note=note)

    def _start_log(self):
        self.nr_episodes, self._log_time, self._log_step = 0, time.time(), 0

    def _episode_stats(self, scalars):
        """the train env's episodes finished since the last call: counted, their means into `scalars` -> (count, mean return)"""
        if not hasattr(self.train_env, "pop_episode_stats"):
            return 0, None
        n_done, mean_ret, mean_len = self.train_env.pop_episode_stats()
        self.nr_episodes += n_done
        if n_done:
            scalars.update({"rollout/episode_return": mean_ret, "rollout/episode_length": mean_len})
        return n_done, mean_ret

    def _sps(self, global_step):
        """env steps per second since the last call"""
        now = time.time()
        sps = int((global_step - self._log_step) / max(now - self._log_time, 1e-9))
        self._log_time, self._log_step = now, global_step
        return sps

    def _write_log(self, global_step, scalars):
        self.sink.write(global_step, scalars)
        self.last_metrics = scalars

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, episodes=None):
        """Deterministic steps on the eval env -> (episode returns, lengths): `horizon` steps (fastsac.py:357-372), or with
        `episodes` until that many have ended, 100 `horizon` steps at the most (reppo.py:413-450)"""
        env, t = self.eval_env, self.torch
        shared = env is self.train_env
        if shared and not hasattr(env, "snapshot"):
            raise ValueError(self._NAME + ": evaluation on the training env needs env.snapshot()/restore(); "
                             "set environment.copy_train_env_for_eval=False")
        snap = env.snapshot() if shared else None
        try:
            state, _ = env.reset()
            ne = state.shape[0]
            ep_ret, ep_len = t.zeros(ne, device=self.device), t.zeros(ne, device=self.device)
            returns, lengths = [], []
            for _ in range(int(self.horizon) * (1 if episodes is None else 100)):
                state, reward, terminated, truncated, info = env.step(self.act(state, deterministic=True))
                ep_ret += reward
                ep_len += 1
                done = terminated | truncated
                if bool(done.any()):
                    returns.extend(ep_ret[done].cpu().tolist())
                    lengths.extend(ep_len[done].cpu().tolist())
                    ep_ret = t.where(done, t.zeros_like(ep_ret), ep_ret)
                    ep_len = t.where(done, t.zeros_like(ep_len), ep_len)
                    if episodes is not None and len(returns) >= episodes:
                        break
            return returns[:episodes], lengths[:episodes]
        finally:
            if shared:
                env.restore(snap)

    def test(self, episodes):
        return self.evaluate()[0][:episodes]       # deterministic inference: acting buffers only

    # ------------------------------------------------------------------ checkpoint
    def _state_names(self):
        return self._STATE + (self._NORM_STATE if self.obs_norm else ())

    def save(self):
        """Native checkpoint: the flat parameter / optimiser-moment vectors of _STATE, the normaliser statistics, the counters, the
        key and the algorithm config (the references store their modules' and optimisers' state_dicts)."""
        path = os.path.join(self.save_path, self._FILE)
        state = {k: getattr(self, k).cpu().numpy() for k in self._state_names()}
        np.savez(path + ".tmp.npz", **{k: getattr(self, k) for k in self._COUNTERS}, key=self.key,
                 config_algorithm=json.dumps(self.config.algorithm.to_dict()), **state)
        os.replace(path + ".tmp.npz", path)

    @classmethod
    def load(cls, config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)
        model = cls(config, train_env, eval_env, run_path, writer)
        for k in model._state_names():
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        for k in cls._COUNTERS:
            setattr(model, k, int(ckpt[k]) if ckpt[k].ndim == 0 else tuple(int(x) for x in ckpt[k]))
        model.key = ckpt["key"].astype(np.uint32)
        model._after_load()
        return model

    def _after_load(self):
        pass
