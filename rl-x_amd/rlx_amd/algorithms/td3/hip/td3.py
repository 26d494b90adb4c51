"""td3.hip -- TD3 whose update runs as hand-written gfx950 kernels (rl-x_amd/csrc/td3.hip).

The reference's TD3 (rl_x/algorithms/td3/flax/td3.py) is its SAC host loop with a deterministic policy: the replay ring
(replay_buffer.py is sac/flax's file) and the uniform warm-up (td3.py:235-237) are the same.  This class therefore derives from
`sac.hip`'s (through EnsembleSAC: the flat back-to-back critics and the checkpoint with its layout check) and keeps its ring,
`_host_indices`, warm-up actions, evaluation loop, `test` and metric sinks.  What it replaces: the policy -- a tanh head of act_dim
outputs (policy.py:22-44) WITH a target copy -- acting (rlx_td3_act_f32: one shape-wide normal draw, td3.py:107-112), the update
call (rlx_td3_update_f32: the critic step, and the policy step with both Polyak updates when global_step % policy_delay == 0,
:264-290), the two optimizer counts with their two schedules (:72-79) and the logged names (:338-340).  There is no entropy
coefficient.  Key schedule: key, policy_key, critic_key = split(PRNGKey(seed), 3) (:60-61).

Not taken over from sac.hip: data-parallel training, the ring source inside the update, kept weight images, the full-jit networks
and observation normalisation -- the flags for them do not exist here.  ddpg.hip is this class with one critic and the joint step."""
import numpy as np

from rlx_amd.algorithms.sac.hip.sac import _lecun_flat
from rlx_amd.algorithms.sac_ensemble import EnsembleSAC
from rlx_amd.algorithms.td3.hip.general_properties import GeneralProperties

METRIC_NAMES = ["loss/q_loss", "gradients/critic_grad_norm", "loss/policy_loss", "q_value/q_value", "gradients/policy_grad_norm"]


def linear_schedule(count, *, anneal, learning_rate, nr_envs, learning_starts, total_timesteps):
    """linear_schedule (td3.py:72-76) at `count` previous steps of the optimiser that asks"""
    if not anneal:
        return learning_rate
    return learning_rate * (1.0 - (count * nr_envs - learning_starts) / (total_timesteps - learning_starts))


class TD3(EnsembleSAC):
    _NAME = "td3.hip"
    NR_CRITICS, JOINT = 2, False
    _STATE = ("pparams", "pm", "pv", "ptarget", "qparams", "qm", "qv", "qtarget")
    # the loop's counts (td3.py:216-217) and the two optax counts (:88, :95)
    _COUNTERS = ("nr_critic_updates", "nr_policy_updates", "q_count", "pi_count")

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        self._refuse(alg)
        self.q_count = self.pi_count = self.nr_critic_updates = self.nr_policy_updates = 0
        super().__init__(config, train_env, eval_env, run_path, writer)
        from rlx_amd.hip import ACT_RELU, mlp_desc
        torch, hiplib = self.torch, self.hiplib
        self.epsilon = float(alg.epsilon)
        self.smoothing_epsilon = 0.0 if self.JOINT else float(alg.smoothing_epsilon)
        self.smoothing_clip_value = 0.0 if self.JOINT else float(alg.smoothing_clip_value)
        self.policy_delay = 1 if self.JOINT else int(alg.policy_delay)
        if self.policy_delay < 1:
            raise ValueError(f"{self._NAME}: policy_delay must be at least 1")
        self.ensemble_size = self.NR_CRITICS
        self.global_step = 0
        # td3.py:60-61: a three-way split (sac.py's is four-way: the entropy coefficient's key is gone)
        self.key, policy_key, critic_key = hiplib.threefry_split(hiplib.prng_key(self.seed), 3, self.scheme)
        H, Op, A = self.nr_hidden_units, self.policy_obs_dim, self.act_dim
        self.pdesc = mlp_desc(Op, [H, H], A, ACT_RELU, False, False)          # policy.py:31-36; the target starts equal (td3.py:86-87)
        prng = np.random.default_rng([int(policy_key[0]), int(policy_key[1])])
        self.pparams = torch.from_numpy(_lecun_flat(prng, Op, [H, H], A)).to(self.device)
        self.ptarget = self.pparams.clone()
        self.pm, self.pv = torch.zeros_like(self.pparams), torch.zeros_like(self.pparams)
        n_in = self.critic_obs_dim + A                                         # critic.py:17-53: each net from its own split of critic_key
        self.qdesc = mlp_desc(n_in, [H, H], 1, ACT_RELU, False, False)
        q = np.concatenate([_lecun_flat(np.random.default_rng([int(k[0]), int(k[1])]), n_in, [H, H], 1)
                            for k in hiplib.threefry_split(critic_key, self.NR_CRITICS, self.scheme)])
        self.nq = q.size // self.NR_CRITICS
        self.qparams = torch.from_numpy(q).to(self.device)
        self.qtarget = self.qparams.clone()
        self.qm, self.qv = torch.zeros_like(self.qparams), torch.zeros_like(self.qparams)
        del self.log_alpha, self.am, self.av

    # the policy's optimizer count under SAC's name: SAC's loop and log line read it
    @property
    def opt_count(self):
        return self.pi_count

    @opt_count.setter
    def opt_count(self, v):
        self.pi_count = int(v)

    def _schedule_args(self):
        return dict(anneal=self.anneal_learning_rate, learning_rate=self.learning_rate, nr_envs=self.nr_envs,
                    learning_starts=self.learning_starts, total_timesteps=self.total_timesteps)

    def current_lr(self):
        return linear_schedule(self.pi_count, **self._schedule_args())       # td3.py:196: the POLICY's rate is the logged one

    def hparams(self, policy_step=True):
        from rlx_amd.hip import Td3Hparams
        return Td3Hparams(self.gamma, self.tau, self.smoothing_epsilon, self.smoothing_clip_value, self.current_lr(),
                          linear_schedule(self.q_count, **self._schedule_args()), 0.9, 0.999, 1e-8, self.NR_CRITICS, int(self.JOINT),
                          int(bool(policy_step)))

    def act(self, obs, action, processed):
        return self.ctx.td3_act(self.pdesc, self.pparams, obs, self.key, action, processed[2], self.env_as_low, self.env_as_high,
                                self.epsilon, self.scheme)

    def act_deterministic(self, obs, action):
        if getattr(self, "_eval_processed", None) is None or self._eval_processed.shape != action.shape:
            self._eval_processed = self.torch.empty_like(action)
        self.ctx.td3_act(self.pdesc, self.pparams, obs, self.key, action, self._eval_processed, self.env_as_low, self.env_as_high, 0.0)
        return self._eval_processed

    def vector_step(self, env, state, warmup=False, gen=None):
        out = super().vector_step(env, state, warmup, gen)
        self.global_step += self.nr_envs                                       # td3.py:256
        return out

    def train(self):
        self.global_step = 0
        self._pi_logged, self._lr_sum, self._lr_logged = self.nr_policy_updates, 0.0, None
        return super().train()

    def policy_step_due(self):
        return self.global_step % self.policy_delay == 0                       # td3.py:266, as written: global_step advances by nr_envs

    def update(self, batch, policy_step=True):
        """update_critic and, with policy_step, update_policy_and_targets (td3.py:278-290) on batch = (states, next_states, actions,
        rewards, terminations): full observation rows, of which the policy's and the critics' columns are selected here when the env
        defines them.  A critic-only call leaves metrics_dev[2:5] at zero."""
        hp = self.hparams(policy_step)
        batch = self._select_columns(batch, hp)
        if policy_step:
            self._lr_sum = getattr(self, "_lr_sum", 0.0) + hp.lr_policy       # td3.py:196: the rate this policy step uses
        else:
            self.metrics_dev[2:5].zero_()
        self.key, self.q_count, self.pi_count = self.ctx.td3_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.ptarget, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget, batch,
            self.key, self.q_count, self.pi_count, hp, self.metrics_dev, self.scheme)
        self.nr_critic_updates += 1
        self.nr_policy_updates += int(bool(policy_step))

    def sample_and_update(self):
        self.idx1, self.idx2 = self._host_indices(self.batch_size, self.nr_envs)      # replay_buffer.py:31-32
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch, self.policy_step_due())

    def named_metrics(self, m, n_updates):
        """the critic's metrics are means over the interval's critic steps, the policy's over its policy steps (td3.py:355)"""
        n_pi = self.nr_policy_updates - getattr(self, "_pi_logged", 0)
        self._pi_logged = self.nr_policy_updates
        self._lr_logged = self._lr_sum / n_pi if n_pi else None
        self._lr_sum = 0.0
        out = {METRIC_NAMES[i]: m[i] for i in range(2)}
        if n_pi:
            out.update({METRIC_NAMES[i]: m[i] * n_updates / n_pi for i in range(2, 5)})
        return out

    def update_counters(self, nr_updates):
        return {"steps/nr_critic_updates": self.nr_critic_updates, "steps/nr_policy_updates": self.nr_policy_updates}   # td3.py:339-340

    def logged_lr(self):
        """the mean, over the interval's policy steps, of the rate each used (td3.py:196, :355); without one: the current rate"""
        lr, self._lr_logged = getattr(self, "_lr_logged", None), None
        return self.current_lr() if lr is None else lr

    def critic_layout(self):
        return {"nr_critics": self.NR_CRITICS, "critic_params_per_net": int(self.nq), "critic_in_dim": int(self.qdesc.in_dim),
                "policy_params": int(self.pparams.numel()), "hidden": [self.nr_hidden_units, self.nr_hidden_units]}

    def _check_layout(self, layout):
        if layout != self.critic_layout():
            raise ValueError(f"{self._NAME}: the checkpoint's layout {layout} does not fit this configuration {self.critic_layout()}")

    def general_properties():
        return GeneralProperties
