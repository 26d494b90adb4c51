"""GPU: the persistent acting kernel (k_rollout_steps, rl-x_amd/csrc/rollout.hip: several acting steps per launch) against the T
launches of k_rollout_step.  Every case runs the same two consecutive rollouts twice from identical state, first with the option
rollout_persistent = 0 and then with 1, through rlx_ppo_rollout_f32: every array, the env state and the key must be equal bit
for bit (the episode statistics, float atomics, to rtol 1e-5), and the launch counters must show which path ran."""
import numpy as np
import pytest
import torch

from oracle import nets
from rlx_amd.hip import mlp_desc

pytestmark = pytest.mark.gpu

FULL_JIT = (512, 256, 128)
T_MOST = 0.5


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Buf:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def _case(N, T, S, O=17, A=6, hidden=FULL_JIT, act=nets.ACT_ELU, ln=True, clip=False, row_off=0, id_off=0, extra_global=0,
          horizon=3, p_term=0.2, gemm_bx=1, persistent_expected=True):
    return dict(N=N, T=T, S=S, O=O, A=A, hidden=hidden, act=act, ln=ln, clip=clip, row_off=row_off, id_off=id_off,
                n_global=N + row_off + extra_global, horizon=horizon, p_term=p_term, gemm_bx=gemm_bx,
                persistent_expected=persistent_expected)


def _run(ctx, dev, c, persistent):
    """two consecutive rollouts (the env clock, the key, the env state and the critic's counter carry over) -> arrays, counters"""
    N, T, O, A = c["N"], c["T"], c["O"], c["A"]
    rng = np.random.default_rng(1000 * N + 10 * O + A)
    ps, cs = nets.MLPSpec(O, list(c["hidden"]), A, c["act"], c["ln"], True), nets.MLPSpec(O, list(c["hidden"]), 1, c["act"], c["ln"], False)
    pp = (nets.init_params(ps, rng, 0.01) + 0.05 * rng.standard_normal(ps.n_params)).astype(np.float32)
    cp = (nets.init_params(cs, rng, 1.0) + 0.05 * rng.standard_normal(cs.n_params)).astype(np.float32)
    pd, cd = mlp_desc(O, c["hidden"], A, c["act"], c["ln"], True), mlp_desc(O, c["hidden"], 1, c["act"], c["ln"], False)
    assert ctx.rollout_step_supported(pd, cd)
    P, C = _t(pp, dev), _t(cp, dev)
    lo, hi = _t(np.linspace(-2.0, -0.5, A).astype(np.float32), dev), _t(np.linspace(0.5, 3.0, A).astype(np.float32), dev)
    obs = _t(rng.standard_normal((N, O)).astype(np.float32), dev)
    env = dict(seed=11, env_id_offset=c["id_off"], horizon=c["horizon"], p_term=c["p_term"], reward_noise=0.1,
               ep_step=_t(rng.integers(0, c["horizon"], N).astype(np.int32), dev), ep_ret=_t(rng.standard_normal(N).astype(np.float32), dev),
               last_ret=torch.zeros(N, device=dev), last_len=torch.zeros(N, device=dev), episode_stats=torch.zeros(4, device=dev))
    ctx.set_option("gemm_bx", c["gemm_bx"])
    ctx.set_option("rollout_persistent", persistent)
    ctx.set_option("rollout_chunk_steps", c["S"])
    try:
        ctx.rollout_begin(pd, P, cd, C)
        before = [ctx.get_counter("ro_persistent_launches"), ctx.get_counter("ro_step_launches")]
        key, out, critic_es = np.array([5, 77], np.uint32), [], []
        for r in range(2):
            states, obs_last = torch.full((T, N, O), -7.0, device=dev), torch.full((N, O), -7.0, device=dev)
            actions, values, logps = (torch.full(s, -7.0, device=dev) for s in ((T, N, A), (T, N), (T, N)))
            fin, rew, term = (torch.full(s, -7.0, device=dev) for s in ((T, N, O), (T, N), (T, N)))
            states[0].copy_(obs)
            key = ctx.rollout(pd, P, cd, C, states, obs_last, key, actions, values, logps,
                              dict(env, t=r * T, final_obs=fin, reward=rew, terminated=term), clip_and_rescale=c["clip"],
                              act_low=lo if c["clip"] else None, act_high=hi if c["clip"] else None,
                              noise_row_offset=c["row_off"], n_global=c["n_global"])
            torch.cuda.synchronize()
            out += [x.cpu().numpy().copy() for x in (states, actions, values, logps, fin, rew, term, obs_last, env["ep_step"],
                                                     env["ep_ret"], env["last_ret"], env["last_len"])] + [np.asarray(key).copy()]
            if persistent and c["persistent_expected"]:      # (the counters' array belongs to the last persistent rollout)
                ptr = ctx.get_counter("ro_critic_es_ptr")
                critic_es.append(torch.as_tensor(_Buf(ptr, N), device=dev).cpu().numpy().copy())
            obs = obs_last
        launches = [ctx.get_counter("ro_persistent_launches") - before[0], ctx.get_counter("ro_step_launches") - before[1]]
        return out, env["episode_stats"].cpu().numpy().copy(), launches, critic_es
    finally:
        ctx.rollout_end()
        ctx.set_option("gemm_bx", 1)
        ctx.set_option("rollout_persistent", 1)
        ctx.set_option("rollout_chunk_steps", 32)


def _compare(ctx, dev, c):
    T, S = c["T"], c["S"]
    ref, ref_stats, ref_launches, _ = _run(ctx, dev, c, 0)
    got, got_stats, got_launches, critic_es = _run(ctx, dev, c, 1)
    assert ref_launches == [0, 2 * T]
    if c["persistent_expected"]:
        assert got_launches == [2 * ((T + S - 1) // S), 0]
    else:
        assert got_launches == [0, 2 * T]
    assert len(ref) == len(got) == 26
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape and np.array_equal(a, b), f"array {i % 13} of rollout {i // 13}"
    np.testing.assert_allclose(got_stats, ref_stats, rtol=1e-5)
    assert all(np.all(np.isfinite(x)) for x in ref[:8]) and not np.any(ref[0] == -7.0) and not np.any(ref[7] == -7.0)
    if c["persistent_expected"]:     # the critic workgroups' private episode-step counters followed the env's
        assert np.array_equal(critic_es[0], got[8]) and np.array_equal(critic_es[1], got[13 + 8])
    return ref


def test_resets_in_consecutive_steps_truncation_and_termination(ctx, dev):
    """N = 33 (two tiles, the second with one valid row), T = 2 S + 3, horizon 3 with termination probability 0.2"""
    c = _case(33, 9, 3)
    ref = _compare(ctx, dev, c)
    states, fin, term, obs_last = ref[0], ref[4], ref[6], ref[7]
    nxt = np.concatenate([states[1:], obs_last[None]])
    done = (nxt != fin).any(axis=2)                        # a reset replaced the next observation
    assert np.array_equal(done | (term > 0.5), done)       # every termination is a reset
    assert (term > 0.5).any() and (done & ~(term > 0.5)).any()          # termination and truncation both occurred
    assert (done[:-1] & done[1:]).any()                                 # one env reset in two consecutive steps
    assert done.any(axis=1).sum() > T_MOST * done.shape[0]              # resets in most steps


@pytest.mark.parametrize("T", [1, 3, 4, 5])
def test_chunk_boundaries_ragged_tiles(ctx, dev, T):
    """N = 300 (ten tiles, ragged), S = 4: T = 1, S - 1, S, S + 1; even obs width, one action, tanh without LayerNorm, two hidden
    layers, clipping"""
    _compare(ctx, dev, _case(300, T, 4, O=12, A=1, hidden=(512, 128), act=nets.ACT_TANH, ln=False, clip=True))


def test_rank_shard_full_widths(ctx, dev):
    """noise_row_offset / env_id_offset != 0 with N_global > N; obs width 32, 12 actions, a 256-wide last layer, clipping"""
    _compare(ctx, dev, _case(70, 5, 2, O=32, A=12, hidden=(512, 128, 256), clip=True, row_off=128, id_off=128, extra_global=131))


def test_default_chunk_longer_than_the_rollout(ctx, dev):
    _compare(ctx, dev, _case(33, 5, 32, act=nets.ACT_TANH))


@pytest.mark.parametrize("what", ["valu_first_layer", "no_images"])
def test_outside_the_envelope_the_step_launches_run(ctx, dev, what):
    """a first layer that is not 512 wide, and gemm_bx = 0 (no weight images): T launches of k_rollout_step, same results"""
    if what == "valu_first_layer":
        _compare(ctx, dev, _case(33, 4, 3, hidden=(256, 128), persistent_expected=False))
    else:
        _compare(ctx, dev, _case(33, 4, 3, gemm_bx=0, persistent_expected=False))
