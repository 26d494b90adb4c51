"""`espo.hip`: the ESPO training loop of rl_x/algorithms/espo/pytorch/espo.py:160-400 around the library's epoch loop
(rl-x_amd/csrc/espo.hip).

ESPO's networks are PPO's two-tanh-layer nets and its acting, next-value and GAE phases are PPO's (espo.py:186-230), so this class
derives from `ppo.hip`'s and keeps its rollout (`collect_rollout`), `compute_advantages`, evaluation and `test` unchanged: the same
library calls (rlx_ppo_rollout_f32 / rlx_actor_critic_fwd_sample_f32, rlx_ppo_next_values_f32, rlx_gae_f32).  What differs is the
optimisation phase: up to max_epochs policy / critic steps on minibatches drawn by `np.random.default_rng(seed).choice`, ended by
the first epoch whose ratio_delta exceeds max_ratio_delta -- ONE rlx_espo_update_f32 call per iteration, which decides the stop on
the device and blocks once, at its end.

Minibatch rows: the reference draws one `choice` per executed epoch (espo.py:241).  All max_epochs draws are uploaded in one array
before the call; afterwards the generator is put back to its state in front of the draws and advanced by the epochs that ran, so
the host stream stays the reference's."""
import json
import logging
import math
import os
import time
import types

import numpy as np

from rlx_amd.algorithms.espo.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.ppo.hip.ppo import PPO
from rlx_amd.environments.data_interface_type import DataInterfaceType
from rlx_amd.plugin import adopt_checkpoint_config
from rlx_amd.runner.config_dict import ConfigDict

rlx_logger = logging.getLogger("rl_x")

METRIC_NAMES = ["loss/policy_gradient_loss", "loss/critic_loss", "loss/entropy_loss", "policy_ratio/ratio_delta",
                "policy_ratio/approx_kl", "gradients/policy_grad_norm", "gradients/critic_grad_norm"]      # espo.py:266-274
DELTA_OPERATORS = {"mean": 0, "median": 1}


class ESPO(PPO):
    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        if alg.device != "gpu":
            raise ValueError("espo.hip runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)")
        if bool(alg.bf16_mixed_precision_training):
            raise ValueError("espo.hip computes in fp32: set --algorithm.bf16_mixed_precision_training=False")
        if alg.delta_calc_operator not in DELTA_OPERATORS:
            raise ValueError("Unknown delta_calc_operator")                         # espo.py:63
        if train_env.general_properties.data_interface_type != DataInterfaceType.TORCH:
            raise ValueError("espo.hip needs a TORCH data-interface environment")
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("espo.hip runs on one GPU")
        except ImportError:
            pass
        self.max_epochs = int(alg.max_epochs)
        self.max_ratio_delta = float(alg.max_ratio_delta)
        self.delta_calc_operator = alg.delta_calc_operator
        batch_size = int(config.environment.nr_envs) * int(alg.nr_steps)
        if self.max_epochs < 1:
            raise ValueError("espo.hip: max_epochs must be at least 1")
        if not 2 <= int(alg.minibatch_size) <= min(4096, batch_size):
            raise ValueError("espo.hip: minibatch_size must be in 2..4096 and at most nr_envs * nr_steps")
        # the base class reads PPO's flag set: ESPO's, plus the values its constructor needs (one 'epoch' over one whole-batch
        # 'minibatch' -- it only derives counts from them; the update below never uses those)
        view = ConfigDict()
        for k, v in alg.items():
            view[k] = v
        view.nr_epochs, view.clip_range, view.network_architecture, view.minibatch_size = 1, 0.0, "flax", batch_size
        super().__init__(types.SimpleNamespace(algorithm=view, environment=config.environment, runner=config.runner), train_env, eval_env,
                         run_path, writer)
        self.config = config
        self.minibatch_size = int(alg.minibatch_size)
        if self.discrete:
            raise ValueError("espo.hip: continuous action spaces only")
        from rlx_amd.hip import EspoHparams
        self.rng = np.random.default_rng(self.seed)                                 # espo.py:79
        self.ehp = EspoHparams(self.max_ratio_delta, float(alg.entropy_coef), float(alg.critic_coef), float(alg.max_grad_norm), 0.9, 0.999,
                               1e-8, DELTA_OPERATORS[self.delta_calc_operator])     # torch.optim.Adam defaults (espo.py:87-88)
        self.nr_iterations = 0          # LinearLR is stepped once per iteration (espo.py:284-286)
        t = self.torch
        self._idx_host = t.empty(self.max_epochs, self.minibatch_size, dtype=t.int32).pin_memory()
        self._idx_dev = t.empty(self.max_epochs, self.minibatch_size, dtype=t.int32, device=self.device)
        self._metrics = t.zeros(self.max_epochs, 8, device=self.device)
        self._no_rows = t.zeros(1, 10, device=self.device)
        self._log = t.zeros(19, device=self.device)

    # ------------------------------------------------------------------ buffers: the update reads the FULL observation rows
    def _alloc_batch(self):
        B = super()._alloc_batch()
        t = self.torch
        B.full_states = (t.zeros(self.nr_steps, self.nr_envs_local, self.obs_dim, device=self.device, dtype=t.float32) if self.obs_select
                         else B.states)
        return B

    def _act(self, batch, state, step):
        if self.obs_select:
            batch.full_states[step].copy_(state)
        super()._act(batch, state, step)

    # ------------------------------------------------------------------ optimisation phase (espo.py:232-294)
    def current_lr(self):
        if not self.anneal_learning_rate:
            return float(self.learning_rate)
        total = max(int(self.total_timesteps // self.batch_size), 1)                # LinearLR(1 -> 0, total_iters), espo.py:91-92
        return float(self.learning_rate) * (1.0 - min(self.nr_iterations, total) / total)

    def update(self, batch, metrics_out=None):
        """-> epochs run.  One library call; the host generator ends where `epochs run` lazy draws would have left it."""
        B, mb, E = self.batch_size, self.minibatch_size, self.max_epochs
        before = self.rng.bit_generator.state
        idx = self._idx_host.numpy()
        for e in range(E):
            idx[e] = self.rng.choice(B, size=mb, replace=False)
        self._idx_dev.copy_(self._idx_host, non_blocking=True)
        O, A = self.obs_dim, self.act_dim
        run, self.opt_count = self.ctx.espo_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.cdesc, self.cparams, self.cm, self.cv, batch.full_states.view(B, O),
            batch.actions.view(B, A), batch.log_probs.view(B), batch.returns.view(B), batch.advantages.view(B), self._idx_dev,
            self.opt_count, self.current_lr(), self.ehp, self._metrics if metrics_out is None else metrics_out,
            pidx=self.pidx if self.obs_select else None, cidx=self.cidx if self.obs_select else None)
        self.rng.bit_generator.state = before
        for _ in range(run):
            self.rng.choice(B, size=mb, replace=False)
        return run

    def reduce_metrics(self, batch, run):
        """means over the executed epochs (espo.py:288), explained variance and the policy's std: one device -> host copy"""
        t = self.torch
        logstd = self.pparams[self.logstd_offset:self.logstd_offset + self.act_dim]
        self.ctx.ppo_reduce_metrics(self._no_rows, batch.returns, batch.values, logstd, self._log[:12])
        self._log[12:] = self._metrics[:run, :7].mean(0)
        host = self._log.cpu().tolist()
        m = host[12:]
        if not all(math.isfinite(v) for v in m):
            raise FloatingPointError("espo.hip: non-finite loss / gradient norm in this iteration " + str([round(v, 6) for v in m]) +
                                     ".  The optimizer steps of the affected epochs were SKIPPED on the device.")
        out = dict(zip(METRIC_NAMES, m))
        out["v_value/explained_variance"], out["policy/std_dev"] = host[10], host[11]
        return out

    def train_iteration(self, batch, state):
        """acting, GAE, the epoch loop -> (next observation, epochs run)"""
        state = self.collect_rollout(batch, state)
        self.compute_advantages(batch)
        return state, self.update(batch)

    def train(self):
        t = self.torch
        self.set_train_mode()
        batch = self._alloc_batch()
        state, _ = self.train_env.reset()
        state = state.contiguous()
        global_step = nr_updates = nr_episodes = 0
        prev_end = None
        ev = [t.cuda.Event(enable_timing=True) for _ in range(4)]
        while global_step < self.total_timesteps:
            lr_now = self.current_lr()
            ev[0].record()
            state = self.collect_rollout(batch, state)
            ev[1].record()
            self.compute_advantages(batch)
            ev[2].record()
            run = self.update(batch)
            ev[3].record()
            self.nr_iterations += 1
            global_step += self.nr_steps * self.nr_envs
            nr_updates += run
            optimization_metrics = self.reduce_metrics(batch, run)
            optimization_metrics["optim/nr_epochs"] = run
            optimization_metrics["lr/learning_rate"] = lr_now if not self.anneal_learning_rate else self.current_lr()
            time_metrics = {"time/acting_time": ev[0].elapsed_time(ev[1]) / 1e3,
                            "time/calc_adv_and_return_time": ev[1].elapsed_time(ev[2]) / 1e3,
                            "time/optimizing_time": ev[2].elapsed_time(ev[3]) / 1e3}
            evaluation_metrics = {}
            if self.evaluation_frequency != -1 and global_step % self.evaluation_frequency == 0:
                t_eval = time.time()
                self.set_eval_mode()
                rets, lens = self.evaluate(self.evaluation_episodes)
                evaluation_metrics = {"eval/episode_return": float(np.mean(rets)), "eval/episode_length": float(np.mean(lens))}
                self.set_train_mode()
                time_metrics["time/evaluating_time"] = time.time() - t_eval
            rollout_info_metrics = {}
            if hasattr(self.train_env, "pop_episode_stats"):
                n_done, mean_ret, mean_len = self.train_env.pop_episode_stats()
                nr_episodes += n_done
                if n_done:
                    rollout_info_metrics = {"rollout/episode_return": mean_ret, "rollout/episode_length": mean_len}
                    if self.save_model and mean_ret > self.best_mean_return:
                        self.best_mean_return = mean_ret
                        self.save()
            now = time.time()
            if prev_end:
                time_metrics["time/sps"] = int((self.nr_steps * self.nr_envs) / (now - prev_end))
            prev_end = now
            steps_metrics = {"steps/nr_env_steps": global_step, "steps/nr_updates": nr_updates, "steps/nr_episodes": nr_episodes}
            combined = {**rollout_info_metrics, **evaluation_metrics, **steps_metrics, **time_metrics, **optimization_metrics}
            self.sink.write(global_step, combined)
            self.last_metrics = combined

    # ------------------------------------------------------------------ checkpoint: PPO's arrays, the counters and the host generator
    def save(self):
        path = os.path.join(self.save_path, self.best_model_file_name)
        state = {k: getattr(self, k).cpu().numpy() for k in ("pparams", "pm", "pv", "cparams", "cm", "cv")}
        np.savez(path + ".tmp.npz", opt_count=self.opt_count, nr_iterations=self.nr_iterations, key=self.key,
                 rng_state=json.dumps(self.rng.bit_generator.state), policy_obs_dim=self.policy_obs_dim,
                 critic_obs_dim=self.critic_obs_dim, act_dim=self.act_dim, config_algorithm=json.dumps(self.config.algorithm.to_dict()),
                 **state)
        os.replace(path + ".tmp.npz", path)

    def load(config, train_env, eval_env, run_path, writer, explicitly_set_algorithm_params):
        ckpt = np.load(config.runner.load_model, allow_pickle=False)
        adopt_checkpoint_config(config, json.loads(str(ckpt["config_algorithm"])), explicitly_set_algorithm_params)
        model = ESPO(config, train_env, eval_env, run_path, writer)
        for k in ("pparams", "pm", "pv", "cparams", "cm", "cv"):
            getattr(model, k).copy_(model.torch.from_numpy(ckpt[k]).to(model.device))
        model.opt_count, model.nr_iterations = int(ckpt["opt_count"]), int(ckpt["nr_iterations"])
        model.key = ckpt["key"].astype(np.uint32)
        model.rng.bit_generator.state = json.loads(str(ckpt["rng_state"]))
        return model

    def general_properties():
        return GeneralProperties
