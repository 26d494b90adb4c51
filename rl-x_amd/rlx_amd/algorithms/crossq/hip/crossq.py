"""crossq.hip -- CrossQ whose updates run as hand-written gfx950 kernels (rl-x_amd/csrc/crossq.hip, brn.hip).

The reference's CrossQ (rl_x/algorithms/crossq/flax/crossq.py) is its SAC host loop over networks whose every Dense is preceded by a
batch renormalisation, WITHOUT target networks: per vector step one critic update over the joint rows [(s, a); (s', a')]
(crossq.py:147-206) and, when global_step % policy_delay == 0, one policy / entropy update on the same batch (:210-274, :345).  This
class derives from EnsembleSAC and keeps sac.hip's warm-up actions, replay ring, `_host_indices`, train loop, evaluation loop and
`test`.  What it replaces: both networks (flat layout bn.scale, bn.bias, W, b per layer, then the last BRN and the head; initial
values scale 1, bias 0, lecun-normal kernels) with their running-statistics vectors (mean 0, var 1), acting (rlx_crossq_act_f32:
the policy in eval mode), the two update calls with their two optimizer counters, and the checkpoint, which carries both
statistics vectors and a critic layout that names the batch renormalisation.  There is no qtarget and no tau.

Not taken over from sac.hip: data-parallel training, the ring source inside the update, kept weight images, the full-jit networks
and observation normalisation -- the flags for them do not exist here, and _refuse raises for them."""
import numpy as np

from rlx_amd.algorithms.crossq.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.sac.hip.sac import _lecun_flat
from rlx_amd.algorithms.sac_ensemble import EnsembleSAC

BRN_EPS, BRN_R_MAX, BRN_D_MAX = 1e-3, 3.0, 5.0                          # batch_renorm.py:80-83


def with_batch_renorm(plain, in_dim, hidden, out_dim):
    """a flat plain network (W, b per layer) -> CrossQ's layout: scale 1 and bias 0 over the layer's INPUT in front of every W"""
    parts, off, d = [], 0, in_dim
    for h in list(hidden) + [out_dim]:
        n = d * h + h
        parts += [np.ones(d, np.float32), np.zeros(d, np.float32), plain[off:off + n]]
        off, d = off + n, h
    return np.concatenate(parts)


def fresh_statistics(in_dim, hidden):
    """mean 0, var 1 for every normalised width: the input, then each hidden layer"""
    return np.concatenate([np.concatenate([np.zeros(d, np.float32), np.ones(d, np.float32)]) for d in [in_dim] + list(hidden)])


def policy_is_due(global_step, policy_delay):
    """crossq.py:345 (after learning has started): the policy is updated when global_step % policy_delay == 0"""
    return global_step % policy_delay == 0


class CrossQ(EnsembleSAC):
    _NAME = "crossq.hip"
    _COUNTERS = ("nr_q_updates", "nr_policy_updates", "global_step")
    _STATE = ("pparams", "pm", "pv", "pstats", "qparams", "qm", "qv", "qstats", "log_alpha", "am", "av")

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = config.algorithm
        self._refuse(alg)
        self._read_crossq(alg)
        super().__init__(config, train_env, eval_env, run_path, writer)
        del self.qtarget, self.tau                                         # no target networks, no Polyak averaging
        self.nr_q_updates, self.global_step = 0, 0
        self._init_networks()

    def _read_crossq(self, alg):
        def width(name):
            v = int(alg[name])
            if v <= 0 or v % 64 != 0 or v > 2048:
                raise ValueError(f"{self._NAME}: {name} must be a multiple of 64, at most 2048")
            return v
        self.ensemble_size = int(alg.ensemble_size)
        if not 1 <= self.ensemble_size <= 16:
            raise ValueError(f"{self._NAME}: ensemble_size must be in 1..16")
        self.policy_delay = int(alg.policy_delay)
        if self.policy_delay < 1:
            raise ValueError(f"{self._NAME}: policy_delay must be at least 1")
        self.policy_width, self.critic_width = width("policy_nr_hidden_units"), width("critic_nr_hidden_units")
        if not 2 <= int(alg.batch_size) < 2 ** 30:
            raise ValueError(f"{self._NAME}: batch_size must be in 2..2^30 - 1 (one row has no batch variance)")
        self.brn_momentum = float(alg.batch_renorm_momentum)
        if not 0.0 <= self.brn_momentum < 1.0:
            raise ValueError(f"{self._NAME}: batch_renorm_momentum must be in [0, 1)")
        self.brn_warmup_steps = int(alg.batch_renorm_warmup_steps)
        if not 0 <= self.brn_warmup_steps < 2 ** 31:
            raise ValueError(f"{self._NAME}: batch_renorm_warmup_steps must be in 0..2^31 - 1")
        self.policy_adam_b1, self.critic_adam_b1 = float(alg.policy_adam_b1), float(alg.critic_adam_b1)

    def _init_networks(self):
        """policy.py:34-72 and critic.py:25-60: each critic from its own split of critic_key, as EnsembleSAC._init_critics does"""
        from rlx_amd.hip import ACT_RELU, mlp_desc
        t, lib = self.torch, self.hiplib
        E, A, Op, n_in = self.ensemble_size, self.act_dim, self.policy_obs_dim, self.critic_obs_dim + self.act_dim
        ph, qh = [self.policy_width] * 2, [self.critic_width] * 2
        self.pdesc, self.qdesc = mlp_desc(Op, ph, 2 * A, ACT_RELU, False, False), mlp_desc(n_in, qh, 1, ACT_RELU, False, False)
        ks = lib.threefry_split(lib.prng_key(self.seed), 4, self.scheme)
        rng = lambda k: np.random.default_rng([int(k[0]), int(k[1])])
        p = with_batch_renorm(_lecun_flat(rng(ks[1]), Op, ph, 2 * A), Op, ph, 2 * A)
        q = np.concatenate([with_batch_renorm(_lecun_flat(rng(k), n_in, qh, 1), n_in, qh, 1) for k in lib.threefry_split(ks[2], E, self.scheme)])
        self.nq = q.size // E
        dev = self.device
        self.pparams, self.qparams = t.from_numpy(p).to(dev), t.from_numpy(q).to(dev)
        self.pstats = t.from_numpy(fresh_statistics(Op, ph)).to(dev)
        self.qstats = t.from_numpy(np.concatenate([fresh_statistics(n_in, qh)] * E)).to(dev)
        self.pm, self.pv = t.zeros_like(self.pparams), t.zeros_like(self.pparams)
        self.qm, self.qv = t.zeros_like(self.qparams), t.zeros_like(self.qparams)
        assert (self.pparams.numel(), self.pstats.numel()) == self.ctx.crossq_counts(self.pdesc)
        assert (self.nq, self.qstats.numel() // E) == self.ctx.crossq_counts(self.qdesc)

    # the policy's / alpha's optimizer counter under SAC's name: SAC's log line and schedule read it
    @property
    def opt_count(self):
        return self.nr_policy_updates

    @opt_count.setter
    def opt_count(self, v):
        self.nr_policy_updates = int(v)

    def hparams(self):
        from rlx_amd.hip.lib import CrossqHparams
        lr = self.current_lr()
        return CrossqHparams(self.gamma, self.target_entropy, self.log_std_min, self.log_std_max, lr, lr, lr, self.policy_adam_b1,
                             self.critic_adam_b1, 0.9, 0.999, 1e-8, self.brn_momentum, BRN_EPS, BRN_R_MAX, BRN_D_MAX, self.brn_warmup_steps,
                             self.ensemble_size)

    # ---- acting: the policy in eval mode (crossq.py:135-143); evaluation: tanh(mean)
    def _act(self, policy_obs, out, deterministic=False):
        self.key = self.ctx.crossq_act(self.pdesc, self.pparams, self.pstats, policy_obs, self.key, out, self.hparams(),
                                       deterministic=deterministic, scheme=self.scheme)

    def vector_step(self, env, state, warmup=False, gen=None):
        """act -> env.step -> replay add; returns the next observation.  Counts the env steps for the policy_delay rule."""
        if warmup:
            action = self.warmup_actions(gen)
        else:
            self._act(self.policy_obs(state.contiguous()), self.action)
            action = self.action
        next_state, reward, terminated, truncated, info = env.step(self.processed_action(action))
        fin = info.get("final_observation") if isinstance(info, dict) else None
        self.replay_add(state, fin if fin is not None else next_state, action, reward, terminated.float())
        self.global_step += self.nr_envs
        return next_state.clone()

    def evaluate(self, episodes):
        """SAC.evaluate with this plugin's acting call: the base class's loop reaches the policy through ctx.sac_act, so the call is
        swapped for its duration"""
        ctx = self.ctx

        class Acting:
            def __getattr__(_, name):
                return getattr(ctx, name)

            def sac_act(_, pdesc, pparams, obs, key, action, *a, deterministic=False, **k):
                key_in = self.key
                self._act(obs, action, deterministic)
                self.key = key_in                                          # evaluation does not advance the training key (sac.py:217-221)
                return key_in

        self.ctx = Acting()
        try:
            return super().evaluate(episodes)
        finally:
            self.ctx = ctx

    # ---- the updates
    def update(self, batch, policy=None):
        """One critic update on batch = (states, next_states, actions, rewards, terminations), then -- when `policy` (default: the
        policy_delay rule at the current global_step) -- the policy / entropy update on the same batch."""
        hp = self.hparams()
        batch = self._select_columns(batch, hp)
        self.key, self.nr_q_updates = self.ctx.crossq_critic_update(
            self.pdesc, self.pparams, self.pstats, self.qdesc, self.qparams, self.qm, self.qv, self.qstats, self.log_alpha, batch, self.key,
            self.nr_q_updates, hp, self.metrics_dev, self.scheme)
        if policy_is_due(self.global_step, self.policy_delay) if policy is None else policy:
            self.key, self.nr_policy_updates = self.ctx.crossq_policy_update(
                self.pdesc, self.pparams, self.pm, self.pv, self.pstats, self.qdesc, self.qparams, self.qstats, self.log_alpha, self.am, self.av,
                batch[0], self.key, self.nr_policy_updates, hp, self.metrics_dev, self.scheme)

    def sample_and_update(self):
        self.idx1, self.idx2 = self._host_indices(self.batch_size, self.nr_envs)
        self.ctx.sac_replay_sample(self.ring, self.idx1, self.idx2, self.batch)
        self.update(self.batch)

    def critic_layout(self):
        return {"ensemble_size": self.ensemble_size, "critic_params_per_net": int(self.nq), "critic_in_dim": int(self.qdesc.in_dim),
                "hidden": [self.critic_width, self.critic_width], "policy_hidden": [self.policy_width, self.policy_width],
                "batch_renorm": {"eps": BRN_EPS, "r_max": BRN_R_MAX, "d_max": BRN_D_MAX, "statistics_per_net": int(self.qstats.numel() // self.ensemble_size)}}

    def _check_layout(self, layout):
        if layout != self.critic_layout():
            raise ValueError(f"{self._NAME}: the checkpoint's critic layout {layout} does not fit this configuration {self.critic_layout()}")

    def general_properties():
        return GeneralProperties
