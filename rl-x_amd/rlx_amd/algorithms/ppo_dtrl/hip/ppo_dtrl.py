"""`ppo_dtrl.hip`: the training loop of rl_x/algorithms/ppo_dtrl/flax_full_jit/ppo_dtrl.py:118-330 around the library's update
(rl-x_amd/csrc/dtrl.hip).

The nets are the full-jit PPO's and so are acting, next values and GAE (ppo_dtrl.py:133-180), so this class derives from `ppo.hip`'s
and keeps its rollout (`collect_rollout`), `compute_advantages`, permutation prefetch, evaluation, `test` and checkpoint unchanged.
What differs is the optimisation phase: ONE rlx_dtrl_update_f32 call per iteration -- nr_epochs x nr_minibatches steps of the loss
with the mean, covariance and entropy projections, each followed by clip + Adam of both networks.  The rollout does not store the
action means: the call computes them from the incoming policy parameters, which nothing has changed since the rollout.
`hip_model.py`'s layer is not used: everything it would provide comes from `ppo.hip`'s class already."""
import logging
import math
import time
import types

import numpy as np

from rlx_amd.algorithms.ppo.hip.ppo import PPO
from rlx_amd.algorithms.ppo_dtrl.hip.general_properties import GeneralProperties
from rlx_amd.environments.data_interface_type import DataInterfaceType
from rlx_amd.runner.config_dict import ConfigDict

rlx_logger = logging.getLogger("rl_x")

METRIC_NAMES = ["loss/policy_gradient_loss", "loss/critic_loss", "loss/entropy_loss", "loss/trust_region_loss", "policy_ratio/approx_kl",
                "policy_ratio/clip_fraction", "projection/eta_mu", "projection/eta_cov", "projection/unprojected_kl_mean",
                "projection/projected_kl_mean", "projection/unprojected_kl_cov", "projection/projected_kl_cov",
                "gradients/policy_grad_norm", "gradients/critic_grad_norm"]          # ppo_dtrl.py:230-243, :291-292


class PPODTRL(PPO):
    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        if alg.device != "gpu":
            raise ValueError("ppo_dtrl.hip runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        if int(alg.nr_parallel_seeds) > 1:
            raise ValueError("ppo_dtrl.hip: nr_parallel_seeds > 1 is not supported (the reference refuses it too, ppo_dtrl.py:74-75)")
        if train_env.general_properties.data_interface_type != DataInterfaceType.TORCH:
            raise ValueError("ppo_dtrl.hip needs a TORCH data-interface environment")
        if not (float(alg.mean_bound) > 0 and float(alg.cov_bound) > 0):
            raise ValueError("ppo_dtrl.hip: mean_bound and cov_bound must be positive")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("ppo_dtrl.hip runs on one GPU")
        except ImportError:
            pass
        # the base class reads PPO's flag set: this plugin's, plus the full-jit nets and PPO's name for the evaluation period
        view = ConfigDict()
        for k, v in alg.items():
            view[k] = v
        view.network_architecture = "full_jit"
        view.evaluation_frequency = int(alg.evaluation_and_save_frequency) if bool(alg.evaluation_active) else -1
        super().__init__(types.SimpleNamespace(algorithm=view, environment=config.environment, runner=config.runner), train_env, eval_env,
                         run_path, writer)
        self.config = config
        if self.discrete:
            raise ValueError("ppo_dtrl.hip: continuous action spaces only")
        if self.minibatch_size < 2:
            raise ValueError("ppo_dtrl.hip: minibatch_size must be at least 2")
        from rlx_amd.hip import DtrlHparams
        self.dhp = DtrlHparams(self.clip_range, self.entropy_coef, self.critic_coef, self.max_grad_norm, 0.9, 0.999, 1e-8,
                               float(alg.mean_bound), float(alg.cov_bound), float(alg.trust_region_coef), float(self.total_timesteps), None)
        self.nr_iterations = 0
        t = self.torch
        self._no_rows = t.zeros(1, 10, device=self.device)
        self._log = t.zeros(12 + len(METRIC_NAMES), device=self.device)

    # ------------------------------------------------------------------ optimisation phase (ppo_dtrl.py:183-300)
    def update(self, batch, metrics_out):
        """One library call.  global_step is the env-step count at the END of this iteration, a float (ppo_dtrl.py:255-257)."""
        self.dhp.critic_states = batch.cstates.data_ptr() if self.obs_select else None
        global_step = float((self.nr_iterations + 1) * self.nr_steps * self.nr_envs)
        self.key, self.opt_count = self.ctx.dtrl_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.cdesc, self.cparams, self.cm, self.cv, batch.states, batch.actions, None,
            batch.log_probs, batch.returns, batch.advantages, self.nr_epochs, self.minibatch_size, self.key, self.opt_count,
            self.lr_schedule(), global_step, self.dhp, metrics_out, self.scheme)

    def reduce_metrics(self, batch, metrics_dev):
        """means over the E*M updates (ppo_dtrl.py:309), explained variance and the policy's std: one device -> host copy"""
        logstd = self.pparams[self.logstd_offset:self.logstd_offset + self.act_dim]
        self.ctx.ppo_reduce_metrics(self._no_rows, batch.returns, batch.values, logstd, self._log[:12])
        self._log[12:] = metrics_dev.mean(0)
        host = self._log.cpu().tolist()
        m = host[12:]
        if not all(math.isfinite(v) for v in m):
            raise FloatingPointError("ppo_dtrl.hip: non-finite loss / gradient norm in this iteration " + str([round(v, 6) for v in m]) +
                                     ".  The optimizer steps of the affected updates were SKIPPED on the device.")
        out = dict(zip(METRIC_NAMES, m))
        out["v_value/explained_variance"], out["policy/std_dev"] = host[10], host[11]
        return out

    def train_iteration(self, batch, state, metrics_out, events=None):
        """acting, GAE, the update -> next observation; the iteration's metrics land in self.last_host_metrics"""
        ev = events or [None] * 4
        rec = lambda e: e.record() if e is not None else None
        rec(ev[0])
        state = self.collect_rollout(batch, state)
        self.prefetch_permutation(rollout_queued=True)
        rec(ev[1])
        self.compute_advantages(batch)
        rec(ev[2])
        self.update(batch, metrics_out)
        rec(ev[3])
        self.nr_iterations += 1
        self.last_host_metrics = self.reduce_metrics(batch, metrics_out)
        return state

    def train(self):
        t = self.torch
        batch = self._alloc_batch()
        n_upd = self.nr_epochs * self.nr_minibatches
        metrics_dev = t.zeros(n_upd, len(METRIC_NAMES), device=self.device)
        state, _ = self.train_env.reset()
        state = state.contiguous()
        global_step = nr_updates = nr_episodes = 0
        prev_end = None
        ev = [t.cuda.Event(enable_timing=True) for _ in range(4)]
        while global_step < self.total_timesteps:
            lr_now = float(self.lr_schedule()[0])
            state = self.train_iteration(batch, state, metrics_dev, ev)
            global_step += self.nr_steps * self.nr_envs
            nr_updates += n_upd
            optimization_metrics = dict(self.last_host_metrics)
            optimization_metrics["lr/learning_rate"] = lr_now
            time_metrics = {"time/acting_time": ev[0].elapsed_time(ev[1]) / 1e3,
                            "time/calc_adv_and_return_time": ev[1].elapsed_time(ev[2]) / 1e3,
                            "time/optimizing_time": ev[2].elapsed_time(ev[3]) / 1e3}
            evaluation_metrics = {}
            if self.evaluation_frequency != -1 and global_step % self.evaluation_frequency == 0:
                t_eval = time.time()
                rets, lens = self.evaluate(self.evaluation_episodes)
                evaluation_metrics = {"eval/episode_return": float(np.mean(rets)), "eval/episode_length": float(np.mean(lens))}
                time_metrics["time/evaluating_time"] = time.time() - t_eval
                if self.save_model:
                    self.save()
            rollout_info_metrics = {}
            if hasattr(self.train_env, "pop_episode_stats"):
                n_done, mean_ret, mean_len = self.train_env.pop_episode_stats()
                nr_episodes += n_done
                if n_done:
                    rollout_info_metrics = {"rollout/episode_return": mean_ret, "rollout/episode_length": mean_len}
            now = time.time()
            if prev_end:
                time_metrics["time/sps"] = int((self.nr_steps * self.nr_envs) / (now - prev_end))
            prev_end = now
            steps_metrics = {"steps/nr_env_steps": global_step, "steps/nr_updates": nr_updates, "steps/nr_episodes": nr_episodes}
            combined = {**rollout_info_metrics, **evaluation_metrics, **steps_metrics, **time_metrics, **optimization_metrics}
            self.sink.write(global_step, combined)
            self.last_metrics = combined

    def load(config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        import json
        from rlx_amd.plugin import adopt_checkpoint_config
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)
        model = PPODTRL(config, train_env, eval_env, run_path, writer)
        for k in ("pparams", "pm", "pv", "cparams", "cm", "cv"):
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        model.opt_count = int(ckpt["opt_count"])
        model.nr_iterations = model.opt_count // max(model.nr_epochs * model.nr_minibatches, 1)
        return model

    def general_properties():
        return GeneralProperties
