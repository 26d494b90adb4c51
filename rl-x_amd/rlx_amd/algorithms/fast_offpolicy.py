"""The pieces FastSAC and FastTD3 share (the reference's two massively-parallel off-policy algorithms use the same ring,
normaliser, learning-rate schedule and evaluation: rl_x/algorithms/fastsac/pytorch and fasttd3/pytorch, replay_buffer.py,
observation_normalizer.py, fastsac.py:93-96 / fasttd3.py:91-93; evaluation fastsac.py:357-372 / fasttd3.py:348-364).

A subclass sets, in its __init__: torch, hiplib (rlx_amd.hip.lib), ctx (rlx_amd.hip.Ctx), device, key, scheme, hp (with .gamma), nr_envs, total_timesteps,
learning_rate, anneal_learning_rate, learning_starts, capacity, n_steps, obs_norm (and then norm_mean / norm_var / norm_std /
norm_count), obs_select (and then pidx), eval_env, train_env, horizon; its _alloc() creates ring, pos, size, idx_t, idx_e, total;
it provides act(state, deterministic) -> the env's action, and the class attribute _NAME (the plugin's name)."""
import numpy as np


class FastOffPolicyLoop:
    _NAME = None

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

    def _columns(self, x, idx, out):
        return self.ctx.select_columns(x, idx, out) if self.obs_select else x

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

    def evaluate(self):
        """`horizon` deterministic steps on the eval env (fastsac.py:357-372) -> (episode returns, lengths)"""
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
            for _ in range(int(self.horizon)):
                state, reward, terminated, truncated, info = env.step(self.act(state, deterministic=True))
                ep_ret += reward
                ep_len += 1
                done = terminated | truncated
                if bool(done.any()):
                    returns.extend(ep_ret[done].cpu().tolist())
                    lengths.extend(ep_len[done].cpu().tolist())
                    ep_ret = t.where(done, t.zeros_like(ep_ret), ep_ret)
                    ep_len = t.where(done, t.zeros_like(ep_len), ep_len)
            return returns, lengths
        finally:
            if shared:
                env.restore(snap)

    def test(self, episodes):
        return self.evaluate()[0][:episodes]       # deterministic inference: acting buffers only (no replay ring)

    _NORM_STATE = ("norm_mean", "norm_var", "norm_std", "norm_count")
