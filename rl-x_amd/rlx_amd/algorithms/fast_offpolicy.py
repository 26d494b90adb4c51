"""The pieces FastSAC, FastTD3, MPO and FastMPO share (the reference's massively-parallel off-policy algorithms use the same ring,
normaliser, learning-rate schedule and evaluation: rl_x/algorithms/fastsac/pytorch and fasttd3/pytorch, replay_buffer.py,
observation_normalizer.py, fastsac.py:93-96 / fasttd3.py:91-93; evaluation fastsac.py:357-372 / fasttd3.py:348-364), on the host
layer of rlx_amd/algorithms/hip_model.py.

`FastOffPolicyLoop`: a subclass sets, in its __init__, hp (with .gamma), learning_rate, anneal_learning_rate, learning_starts,
capacity, n_steps and obs_norm (and then calls _alloc_normalizer); its _alloc() calls _alloc_ring; it provides
act(state, deterministic) -> the env's action.

`TwoPhaseLoop`: the whole loop of the two algorithms that alternate critic steps and a policy step, FastSAC and FastTD3."""
import numpy as np

from rlx_amd.algorithms.hip_model import HipModel, eval_means


class FastOffPolicyLoop(HipModel):
    def current_lr(self, step_index):
        """LinearLR(start 1, end 0, total_iters = total_timesteps // nr_envs - learning_starts), stepped once per vector step that
        optimises (fastsac.py:93-96, :347-350)."""
        if not self.anneal_learning_rate:
            return self.learning_rate
        total = max(self.total_timesteps // self.nr_envs - self.learning_starts, 1)
        return self.learning_rate * max(1.0 - min(step_index, total) / total, 0.0)

    def normalize(self, obs, out, update):
        """ObservationNormalizer.normalize (observation_normalizer.py:26-33)."""
        if not self.obs_norm:
            return obs
        if update:
            self.ctx.obs_norm_update(obs, self.norm_mean, self.norm_var, self.norm_std, self.norm_count)
        return self.ctx.obs_norm_apply(obs, self.norm_mean, self.norm_std, out)

    def _final_next_state(self, next_state, done, info):
        """the observation an episode ENDED on where `done`, not the first one of the next episode that an auto-resetting env
        returns (mpo.py:309-313 actual_next_state; fastmpo.py:247 env_state.actual_next_observation)"""
        t = self.torch
        dev = lambda x: (x if t.is_tensor(x) else t.from_numpy(np.ascontiguousarray(np.asarray(x)))).to(self.device, t.float32)
        fin = info.get("final_observation") if isinstance(info, dict) else None
        if fin is not None and tuple(np.shape(fin)) == tuple(next_state.shape):
            return t.where(done[:, None], dev(fin), next_state)
        out = next_state.clone()
        for i in t.nonzero(done).flatten().tolist():
            out[i] = dev(self.train_env.get_final_observation_at_index(info, i))
        return out

    def _alloc_ring(self, T):
        """the replay ring, and the index vectors and the batch (`total`) of a sample of T rows -> the tensors' keyword arguments"""
        t, N, O, A, cap = self.torch, self.nr_envs, self.obs_dim, self.act_dim, self.capacity
        f = dict(device=self.device, dtype=t.float32)
        self.ring = (t.zeros(cap, N, O, **f), t.zeros(cap, N, O, **f), t.zeros(cap, N, A, **f), t.zeros(cap, N, **f), t.zeros(cap, N, **f),
                     t.zeros(cap, N, **f))                                # states, next_states, actions, rewards, dones, truncations
        self.pos = self.size = 0
        self.total = (t.empty(T, O, **f), t.empty(T, O, **f), t.empty(T, A, **f)) + tuple(t.empty(T, **f) for _ in range(4))
        self.idx_t, self.idx_e = t.empty(T, dtype=t.int32, device=self.device), t.empty(T, dtype=t.int32, device=self.device)
        return f

    def replay_add(self, state, next_state, action, reward, done, truncated):     # replay_buffer.py:23-31
        for dst, src in zip(self.ring, (state, next_state, action, reward, done, truncated)):
            dst[self.pos].copy_(src)
        self.pos = (self.pos + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def sample(self):
        """ReplayBuffer.sample(total_batch_size) (replay_buffer.py:34-96): index draws on the device from the key."""
        if self.n_steps == 1:
            max_start = self.size
        else:
            max_start = self.capacity if self.size >= self.capacity else max(1, self.size - self.n_steps + 1)
        ks = self.hiplib.threefry_split(self.key, 2, self.scheme)
        self.key = ks[0]
        self.ctx.sac_replay_draw(ks[1], self.idx_t.numel(), max_start, self.nr_envs, self.idx_t, self.idx_e, self.scheme)
        self.ctx.fastsac_replay_sample(self.ring, self.n_steps, self.hp.gamma, self.pos, self.size, self.idx_t, self.idx_e, self.total)


class TwoPhaseLoop(FastOffPolicyLoop):
    """FastSAC's and FastTD3's loop (fastsac.py:243-470, fasttd3.py:228-446; the line numbers below are fastsac.py's).  Per vector
    step: act on the normalised observation (statistics frozen), env.step, ring add.  Once `learning_starts` steps are in the ring:
    ONE sample of nr_policy_updates * nr_critic_updates * batch_size transitions, the observation normaliser updated on the sampled
    states and then on the next states, and for every policy update its critic updates and then the policy step on the LAST
    critic slice's states.

    A plugin provides _networks(alg, rng) (pdesc, qdesc, pparams, qparams, hp's own fields and whatever else it learns), act or
    act_pair, _critic_step and _policy_step, and the class attributes CRITIC_METRICS / POLICY_METRICS (the names of the two metric
    vectors' entries, None for one that is not logged) and _LR_FIELDS (hp's learning rates: all follow one schedule)."""
    _COUNTERS = ("critic_count", "policy_count")
    _SKIPPED = (" (the optimizer steps of the affected updates were skipped on the device; no checkpoint was written over the last "
                "good one)")

    def __init__(self, config, train_env, eval_env, run_path, writer):
        alg = self._read_flags(config, train_env, eval_env, run_path, writer)
        self.learning_rate, self.anneal_learning_rate = float(alg.learning_rate), bool(alg.anneal_learning_rate)
        self.batch_size, self.capacity = int(alg.batch_size), int(alg.buffer_size_per_env)
        self.learning_starts, self.n_steps = int(alg.learning_starts), int(alg.n_steps)
        self.nr_critic_updates, self.nr_policy_updates = int(alg.nr_critic_updates_per_policy_update), int(alg.nr_policy_updates_per_step)
        self.logging_frequency, self.evaluation_frequency = int(alg.logging_frequency), int(alg.evaluation_frequency)
        self.save_frequency = int(alg.save_frequency)
        self.obs_norm = bool(alg.enable_observation_normalization)
        if self.logging_frequency % self.nr_envs != 0:                                        # :60-61
            raise ValueError("The logging frequency must be a multiple of the number of environments.")
        if self.save_frequency != -1 and self.save_frequency % self.nr_envs != 0:             # :63-64
            raise ValueError("The save frequency must be a multiple of the number of environments.")
        if float(alg.max_grad_norm) != -1.0 and float(alg.max_grad_norm) <= 0.0:
            raise ValueError(self._NAME + ": max_grad_norm must be -1 (off, the reference's sentinel) or positive")
        self._open_device()
        self._action_bounds()
        self._networks(alg, np.random.default_rng(self.seed))
        self.qtarget = self.qparams.clone()                             # critic.py:19-20
        z = self.torch.zeros_like
        self.pm, self.pv, self.qm, self.qv = z(self.pparams), z(self.pparams), z(self.qparams), z(self.qparams)
        self.critic_count = self.policy_count = 0
        self._alloc_normalizer()
        # max_grad_norm -1: off; else torch clip_grad_norm_ semantics (:129-130, :218-219)
        for k in ("gamma", "tau", "v_min", "v_max", "weight_decay", "max_grad_norm"):
            setattr(self.hp, k, float(alg[k]))
        self.hp.adam_eps = 1e-8
        self.hp.nr_atoms, self.hp.clipped_double_q = int(alg.nr_atoms), int(bool(alg.clipped_double_q_learning))

    # ------------------------------------------------------------------ pieces
    def _alloc(self):
        """Training buffers: the replay ring, the sampled batch, metric accumulators.  (Acting buffers are per batch size:
        _act_buffers -- test() / evaluate() need only those.)"""
        t, T = self.torch, self.nr_policy_updates * self.nr_critic_updates * self.batch_size
        f = self._alloc_ring(T)
        if self.obs_select:
            Op, Oc = self.policy_obs_dim, self.critic_obs_dim
            self.sel = (t.empty(T, Op, **f), t.empty(T, Op, **f), t.empty(T, Oc, **f), t.empty(T, Oc, **f))
        nc, npol = len(self.CRITIC_METRICS), len(self.POLICY_METRICS)
        self.metrics_c, self.metrics_p = t.zeros(nc, **f), t.zeros(npol, **f)
        # sums over the policy updates since the last log (the reference appends one metrics entry per policy update, each with
        # that block's last critic metrics, and averages them all: fastsac.py:300-345, fasttd3.py:326-337)
        self.sum_c, self.sum_p, self.n_met = t.zeros(nc, **f), t.zeros(npol, **f), 0

    def _policy_input(self, state):
        """normalize(update=False) and the policy's columns (:252-253) -> (the policy's input, action buffer, processed-action buffer)"""
        n = int(state.shape[0])
        act_norm, action, processed = self._act_buffers(n)
        x = self.normalize(state.contiguous(), act_norm, False)
        if self.obs_select:
            pobs = self.__dict__.setdefault("_pobs_bufs", {})
            if n not in pobs:
                pobs[n] = self.torch.empty(n, self.policy_obs_dim, device=self.device, dtype=self.torch.float32)
            x = self.ctx.select_columns(x, self.pidx, pobs[n])
        return x, action, processed

    def act_pair(self, state, deterministic=False):
        """(action for the ring, action for the env): one and the same unless the plugin processes it"""
        action = self.act(state, deterministic)
        return action, action

    def optimize(self, step_index):
        """fastsac.py:281-350 / fasttd3.py:296-341 for one vector step"""
        self.sample()
        s, s2 = self.total[0], self.total[1]
        self.normalize(s, s, True)                     # total_normalized_states (update=True), then the next states (:286-287)
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
        for k in self._LR_FIELDS:
            setattr(self.hp, k, lr)
        B = self.batch_size
        for i in range(self.nr_policy_updates):
            for j in range(self.nr_critic_updates):
                o = (i * self.nr_critic_updates + j) * B
                rows = slice(o, o + B)
                batch = (sp[rows], s2p[rows]) + tuple(x[rows] for x in self.total[2:])
                self._critic_step(batch, None if sc is None else sc[rows], None if s2c is None else s2c[rows])
            self._policy_step(sp[rows], None if sc is None else sc[rows])
            self.sum_c += self.metrics_c            # one entry per policy update (device adds, no synchronisation)
            self.sum_p += self.metrics_p
            self.n_met += 1

    def _checked_means(self):
        """mean metrics since the last log as one host list, critic then policy; raises on a non-finite value -- called before a
        checkpoint is written and before logging, so a poisoned state never replaces the last good file"""
        return self._mean_metrics(self.sum_c, self.sum_p, note=self._SKIPPED)

    # ------------------------------------------------------------------ training loop
    def _reset(self):
        """the training buffers and the env's first state"""
        self._alloc()
        state, _ = self.train_env.reset()
        return state.clone()

    def _vector_step(self, state):
        """act, env.step, ring add (:247-268) -> (next state, done flags)"""
        action, processed = self.act_pair(state)
        next_state, reward, terminated, truncated, info = self.train_env.step(processed)
        done = (terminated | truncated).float()
        self.replay_add(state, next_state, action, reward, done, truncated.float())                 # :262
        return next_state.clone(), done

    def train(self):
        state = self._reset()
        global_step = opt_steps = 0
        self._start_log()
        while global_step < self.total_timesteps:
            state, _ = self._vector_step(state)
            global_step += self.nr_envs
            if global_step > self.learning_starts * self.nr_envs:                                   # :273
                self.optimize(opt_steps)
                opt_steps += 1
            if self.evaluation_frequency != -1 and global_step % self.evaluation_frequency == 0:
                self.last_eval = eval_means(*self.evaluate())
            if self.save_model and self.n_met and self.save_frequency != -1 and global_step % self.save_frequency == 0:
                self._checked_means()           # finite BEFORE the file is replaced
                self.save()
            if global_step % self.logging_frequency == 0 or global_step >= self.total_timesteps:
                combined = {}
                if self.n_met:                                                                   # one D2H per logging interval
                    combined.update({k: v for k, v in zip(self.CRITIC_METRICS + self.POLICY_METRICS, self._checked_means()) if k})
                self._episode_stats(combined)
                combined.update(getattr(self, "last_eval", {}))
                combined.update({"steps/nr_env_steps": global_step, "steps/nr_critic_updates": self.critic_count,
                                 "steps/nr_policy_updates": self.policy_count, "steps/nr_episodes": self.nr_episodes,
                                 "lr/learning_rate": self.current_lr(opt_steps), "time/sps": self._sps(global_step)})
                self.sum_c.zero_()
                self.sum_p.zero_()
                self.n_met = 0
                self._write_log(global_step, combined)
