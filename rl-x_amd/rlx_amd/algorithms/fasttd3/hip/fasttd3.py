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
import numpy as np

from rlx_amd.algorithms.fast_offpolicy import TwoPhaseLoop
from rlx_amd.algorithms.fasttd3.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.hip_model import torch_linear_flat

POLICY_HIDDEN = (512, 256, 128)      # policy.py:38-47
CRITIC_HIDDEN = (1024, 512, 256)     # q_network.py:28-36
CRITIC_METRICS = ("loss/q_loss", "q/q_min", "q/q_max", "gradients/critic_grad_norm")
POLICY_METRICS = ("loss/policy_loss", "gradients/policy_grad_norm")


class FastTD3(TwoPhaseLoop):
    _NAME = "fasttd3.hip"
    _STATE = ("pparams", "pm", "pv", "qparams", "qm", "qv", "qtarget")
    CRITIC_METRICS, POLICY_METRICS = CRITIC_METRICS, POLICY_METRICS
    _LR_FIELDS = ("lr_policy", "lr_critic")

    def _networks(self, alg, rng):
        from rlx_amd.hip import FastTd3Hparams, relu_mlp_desc
        torch, A, NA = self.torch, self.act_dim, int(alg.nr_atoms)
        self.noise_std_min, self.noise_std_max = float(alg.noise_std_min), float(alg.noise_std_max)
        self.clip_and_rescale = bool(alg.action_clipping_and_rescaling)
        self.pdesc = relu_mlp_desc(self.policy_obs_dim, POLICY_HIDDEN, A)
        self.qdesc = relu_mlp_desc(self.critic_obs_dim + A, CRITIC_HIDDEN, NA)
        self.pparams = torch.from_numpy(torch_linear_flat(rng, self.policy_obs_dim, POLICY_HIDDEN, A, False, head_std=0.01)).to(self.device)
        q = np.concatenate([torch_linear_flat(rng, self.critic_obs_dim + A, CRITIC_HIDDEN, NA, False) for _ in range(2)])
        self.qparams = torch.from_numpy(q).to(self.device)
        self.hp = FastTd3Hparams()
        self.hp.smoothing_epsilon, self.hp.smoothing_clip_value = float(alg.smoothing_epsilon), float(alg.smoothing_clip_value)
        self.hp.adam_b1, self.hp.adam_b2 = 0.9, 0.999                   # torch.optim.AdamW defaults (fasttd3.py:88-89)

    def _alloc(self):
        super()._alloc()
        self.noise_scales = self.torch.empty(self.nr_envs, device=self.device, dtype=self.torch.float32)

    def act_pair(self, state, deterministic=False):
        """normalize(update=False) + policy.get_action (fasttd3.py:262-264) -> (action for the ring, processed action for the env)"""
        x, action, processed = self._policy_input(state)
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

    def _reset(self):
        state = super()._reset()
        self.redraw_noise_scales()                                      # fasttd3.py:241
        return state

    def _vector_step(self, state):
        """the ring gets the UNclipped action (fasttd3.py:272); the envs whose episode ended get new noise scales (:274-278)"""
        next_state, done = super()._vector_step(state)
        self.redraw_noise_scales(done)
        return next_state, done

    def _critic_step(self, batch, critic_states, critic_next_states):
        """one critic update and its Polyak step (fasttd3.py:312-318)"""
        self.key, self.critic_count = self.ctx.fasttd3_critic_update(
            self.pdesc, self.pparams, self.qdesc, self.qparams, self.qm, self.qv, self.qtarget, batch, self.key, self.critic_count,
            self.hp, self.metrics_c, self.scheme, critic_states=critic_states, critic_next_states=critic_next_states)

    def _policy_step(self, states, critic_states):
        """the policy update on the last critic slice's states (fasttd3.py:320-324)"""
        self.policy_count = self.ctx.fasttd3_policy_update(
            self.pdesc, self.pparams, self.pm, self.pv, self.qdesc, self.qparams, states, self.policy_count, self.hp, self.metrics_p,
            critic_states=critic_states)

    def general_properties():
        return GeneralProperties
