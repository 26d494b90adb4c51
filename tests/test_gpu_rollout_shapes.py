"""GPU: the fused acting step (k_rollout_step, rl-x_amd/csrc/rollout.hip) across the shapes rlx_ppo_rollout_step_supported
accepts -- the cases of rollout_cases.py, whose inputs test_rollout_cases.py qualifies -- against the float64 oracle, with the bars
of test_gpu_rollout.py (rollout_cases.BARS), and the entry point's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import rollout_cases as rc
from oracle import nets, prng
from rlx_amd.hip import lib as L
from rlx_amd.hip import mlp_desc

pytestmark = pytest.mark.gpu

PAD, SENT, ISENT = 32, -777.25, -12345        # rows behind row N of every output, and what they are filled with
RLX_EINVAL, RLX_EUNSUP = -1, -4


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _close(name, got, exp, worst=None):
    """worst: a dict that keeps the largest fraction of each bar seen (printed by the caller)"""
    rtol, atol = rc.BARS[name]
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), rc.bar_fraction(name, got, exp))
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=atol, err_msg=name)


class Device:
    """device copies of a case: parameters, bounds, and every output with PAD sentinel rows behind row N (the kernel is handed
    the first N rows)"""

    def __init__(self, c, dev, env=None):
        N, O, A = c.N, c.O, c.A
        self.c, self.dev = c, dev
        self.P, self.C, self.lo, self.hi = _t(c.pp, dev), _t(c.cp, dev), _t(c.lo, dev), _t(c.hi, dev)
        shapes = dict(action=(A,), processed=(A,), value=(), logp=(), obs_a=(O,), obs_b=(O,), final_obs=(O,), reward=(), terminated=(),
                      ep_ret=(), last_ret=(), last_len=())
        self.full = {k: torch.full((N + PAD,) + s, SENT, device=dev) for k, s in shapes.items()}
        self.full["ep_step"] = torch.full((N + PAD,), ISENT, device=dev, dtype=torch.int32)
        for k, v in self.full.items():
            setattr(self, k, v[:N])
        for k in ("ep_ret", "last_ret", "last_len"):
            getattr(self, k).zero_()
        if env is not None:
            self.obs_a.copy_(_t(env.obs, dev))
            self.ep_step.copy_(_t(env.ep_step, dev))
        self.stats = torch.zeros(4, device=dev)

    def env_args(self, t):
        return dict(seed=rc.ENV["seed"], env_id_offset=rc.ENV["env_id_offset"], t=t, horizon=rc.ENV["horizon"], p_term=rc.ENV["p_term"],
                    reward_noise=rc.ENV["reward_noise"], final_obs=self.final_obs, reward=self.reward, terminated=self.terminated,
                    ep_step=self.ep_step, ep_ret=self.ep_ret, last_ret=self.last_ret, last_len=self.last_len, episode_stats=self.stats)

    def step_kw(self, scheme):
        c = self.c
        return dict(clip_and_rescale=c.clip, act_low=self.lo if c.clip else None, act_high=self.hi if c.clip else None, scheme=scheme,
                    noise_row_offset=rc.NOISE_ROW_OFFSET, n_global=c.n_global)

    def engine(self, ctx, images):
        """explicitly, in every run: the context remembers images by parameter address, and the allocator reuses addresses"""
        c = self.c
        if images:
            before = ctx.get_counter("bx_window_fallbacks")
            assert ctx.get_counter("gemm_bx") != 0
            ctx.rollout_begin(c.pd, self.P, c.cd, self.C)
            assert ctx.get_counter("bx_window_fallbacks") == before      # the images were laid out, not skipped
        else:
            ctx.rollout_end()

    def untouched_past_row_n(self):
        N = self.c.N
        for k, v in self.full.items():
            assert bool((v[N:] == (ISENT if k == "ep_step" else SENT)).all()), k


VARIANTS = [(n, im, s) for n in rc.NAMES for im, s in rc.Case(n).variants()]


@pytest.mark.parametrize("name,images,scheme", VARIANTS,
                         ids=[f"{n}-{'fp16-pipe' if im else 'fp32'}-scheme{s}" for n, im, s in VARIANTS])
def test_every_case_matches_the_oracle(ctx, dev, name, images, scheme):
    c = rc.Case(name)
    assert ctx.rollout_step_supported(c.pd, c.cd) and c.supported()
    env = c.env()
    d = Device(c, dev, env)
    d.engine(ctx, images)
    processed = d.processed if c.clip else None
    key, ndone, worst = c.key, 0, {}
    obs_in, obs_out = d.obs_a, d.obs_b
    for t in range(rc.STEPS):
        obs = obs_in.cpu().numpy()            # the nets are compared on IDENTICAL inputs (the env's own parity is asserted below)
        new_key = ctx.rollout_step(c.pd, d.P, c.cd, d.C, obs_in, obs_out, key, d.action, processed, d.value, d.logp,
                                   env=d.env_args(t), **d.step_kw(scheme))
        key_e, eps = c.noise(key, scheme)
        assert np.array_equal(new_key, key_e)
        exp = c.expected(obs, eps)
        _close("value", d.value.cpu().numpy(), exp["value"], worst)
        _close("action", d.action.cpu().numpy(), exp["action"], worst)
        _close("logp", d.logp.cpu().numpy(), exp["logp"], worst)
        if c.clip:
            _close("processed", processed.cpu().numpy(), exp["processed"], worst)
            p_dev = processed.cpu().numpy()
        else:
            p_dev = d.action.cpu().numpy()
        # env transition driven by the device's own processed action (identical inputs on both sides)
        obs_e, fin_e, r_e, term_e, _, done_e = env.step(p_dev)
        _close("reward", d.reward.cpu().numpy(), r_e, worst)
        assert np.array_equal(d.terminated.cpu().numpy() > 0.5, term_e)
        _close("obs", d.final_obs.cpu().numpy(), fin_e, worst)
        _close("obs", obs_out.cpu().numpy(), obs_e, worst)
        assert np.array_equal(d.ep_step.cpu().numpy(), env.ep_step)
        ndone += int(done_e.sum())
        key = new_key
        obs_in, obs_out = obs_out, obs_in
    print(f"{name} images={images} scheme={scheme}: fraction of each bar on the device: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert ndone > 0 and d.stats[0].item() == ndone
    if not c.clip:
        assert bool((d.full["processed"] == SENT).all())
    d.untouched_past_row_n()
    ctx.rollout_end()


def test_without_the_env_the_step_returns_after_the_log_prob(ctx, dev):
    """fuse_env = 0: action, value, log-prob and processed action as before, no observation written"""
    c = rc.Case("valu_ln_relu")
    env = c.env()
    d = Device(c, dev, env)
    d.engine(ctx, False)
    obs = d.obs_a.cpu().numpy()
    new_key = ctx.rollout_step(c.pd, d.P, c.cd, d.C, d.obs_a, None, c.key, d.action, d.processed, d.value, d.logp, env=None, **d.step_kw(1))
    key_e, eps = c.noise(c.key, 1)
    assert np.array_equal(new_key, key_e)
    exp = c.expected(obs, eps)
    first = {k: getattr(d, k).cpu().numpy() for k in ("action", "processed", "value", "logp")}
    for k, v in first.items():
        _close(k, v, exp[k])
    # the same call with a buffer in obs_out's place: the same bits, and the buffer keeps its fill
    ctx.rollout_step(c.pd, d.P, c.cd, d.C, d.obs_a, d.obs_b, c.key, d.action, d.processed, d.value, d.logp, env=None, **d.step_kw(1))
    for k, v in first.items():
        assert np.array_equal(getattr(d, k).cpu().numpy(), v), k
    for k in ("obs_b", "final_obs", "reward", "terminated"):
        assert bool((d.full[k] == SENT).all()), k
    assert np.array_equal(d.ep_step.cpu().numpy(), env.ep_step) and d.stats.abs().sum().item() == 0
    d.untouched_past_row_n()


@pytest.mark.parametrize("name", ["three_valu", "mfma_two"])       # one clipped, one unclipped
def test_fused_equals_the_unfused_kernels(ctx, dev, name):
    """rlx_actor_critic_fwd_sample_f32 + rlx_env_step_f32 with the same key: two fp32-accurate evaluations, the bars apply"""
    c = rc.Case(name)
    f, u = Device(c, dev, c.env()), Device(c, dev, c.env())
    f.engine(ctx, False)
    trunc = torch.empty(c.N, device=dev)
    kf = ku = c.key
    fo_in, fo_out = f.obs_a, f.obs_b
    for t in range(rc.STEPS):
        u.obs_a.copy_(fo_in)          # the unfused env steps its observation in place: both sides start the step from the same one
        kf = ctx.rollout_step(c.pd, f.P, c.cd, f.C, fo_in, fo_out, kf, f.action, f.processed, f.value, f.logp, env=f.env_args(t),
                              **f.step_kw(1))
        ku = ctx.actor_critic_fwd_sample(c.pd, u.P, c.cd, u.C, u.obs_a, ku, u.action, u.processed, u.value, u.logp,
                                         clip_and_rescale=c.clip, act_low=u.lo if c.clip else None, act_high=u.hi if c.clip else None,
                                         scheme=1, env_id_offset=rc.NOISE_ROW_OFFSET, n_global=c.n_global)
        assert np.array_equal(kf, ku)
        for k in ("action", "processed", "value", "logp"):
            _close(k, getattr(f, k).cpu().numpy(), getattr(u, k).cpu().numpy().astype(np.float64))
        # the env on the FUSED side's processed action (identical inputs)
        e = rc.ENV
        ctx.env_step(e["seed"], e["env_id_offset"], t, e["horizon"], e["p_term"], e["reward_noise"], f.processed, u.obs_a, u.final_obs,
                     u.reward, u.terminated, trunc, u.ep_step, u.ep_ret, u.last_ret, u.last_len, u.stats)
        _close("reward", f.reward.cpu().numpy(), u.reward.cpu().numpy().astype(np.float64))
        assert torch.equal(f.terminated, u.terminated) and torch.equal(f.ep_step, u.ep_step)
        _close("obs", f.final_obs.cpu().numpy(), u.final_obs.cpu().numpy().astype(np.float64))
        _close("obs", fo_out.cpu().numpy(), u.obs_a.cpu().numpy().astype(np.float64))
        fo_in, fo_out = fo_out, fo_in
    assert f.stats[0].item() == u.stats[0].item() > 0
    f.untouched_past_row_n()
    u.untouched_past_row_n()


def test_one_call_equals_the_step_calls_bit_for_bit(ctx, dev):
    """rlx_ppo_rollout_f32 against T rlx_ppo_rollout_step_f32 calls at a network other than the plugin's defaults, with clipping
    and on the weight images"""
    c = rc.Case("valu_ln_relu")
    T, N, O, A = rc.STEPS, c.N, c.O, c.A
    res = []
    for one_call in (True, False):
        env = c.env()
        d = Device(c, dev, env)
        d.engine(ctx, True)
        states, obs_last = torch.empty(T, N, O, device=dev), torch.empty(N, O, device=dev)
        actions, values, logps = torch.empty(T, N, A, device=dev), torch.empty(T, N, device=dev), torch.empty(T, N, device=dev)
        fin, rew, term = torch.empty(T, N, O, device=dev), torch.empty(T, N, device=dev), torch.empty(T, N, device=dev)
        states[0].copy_(d.obs_a)
        ea = d.env_args(0)
        if one_call:
            key = ctx.rollout(c.pd, d.P, c.cd, d.C, states, obs_last, c.key, actions, values, logps,
                              dict(ea, final_obs=fin, reward=rew, terminated=term), **d.step_kw(1))
        else:
            key = c.key
            for t in range(T):
                key = ctx.rollout_step(c.pd, d.P, c.cd, d.C, states[t], states[t + 1] if t + 1 < T else obs_last, key, actions[t],
                                       None, values[t], logps[t], env=dict(ea, t=t, final_obs=fin[t], reward=rew[t], terminated=term[t]),
                                       **d.step_kw(1))
        res.append([x.cpu().numpy().copy() for x in (states, obs_last, actions, values, logps, fin, rew, term, d.ep_step, d.ep_ret,
                                                     d.last_ret, d.last_len)] + [np.asarray(key), d.stats[0].item()])
    ctx.rollout_end()
    assert res[0][-1] == res[1][-1] > 0
    for a, b in zip(res[0][:-1], res[1][:-1]):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(res[0][2])) and np.any(res[0][0][1] != res[0][0][0])


# --------------------------------------------------------------------------------------------------------------- the refusals
def _raw_step(ctx, d, pd, cd, key, n_global=None, clip=False, lo=None, hi=None, fuse_env=1, final_obs="own"):
    """rlx_ppo_rollout_step_f32 itself, with the caller's key array (the binding hands the library a copy) -> return code"""
    f, c = torch.float32, d.c
    p = lambda x, dt=f: L._ptr(x, dt, True)
    e = d.env_args(0)
    fin = e["final_obs"] if final_obs == "own" else final_obs
    return ctx.lib.rlx_ppo_rollout_step_f32(
        ctx.h, ctypes.byref(pd), p(d.P), ctypes.byref(cd), p(d.C), p(d.obs_a), p(d.obs_b), key, 1, p(d.action), p(d.processed), p(d.value),
        p(d.logp), c.N, int(clip), p(lo), p(hi), rc.NOISE_ROW_OFFSET, int(c.n_global if n_global is None else n_global), fuse_env,
        e["seed"], e["env_id_offset"], 0, e["horizon"], e["p_term"], e["reward_noise"], p(fin), p(e["reward"]), p(e["terminated"]),
        p(e["ep_step"], torch.int32), p(e["ep_ret"]), p(e["last_ret"]), p(e["last_len"]), p(e["episode_stats"]), L._stream())


#            what                                  policy (in, hidden, out, logstd)   critic (in, hidden, out)
UNSUPPORTED = [
    ("no hidden layer", (5, (), 9, True), (5, (), 1)),
    ("four hidden layers", (5, (192, 128, 128, 128), 9, True), (5, (192, 128, 128, 128), 1)),
    ("in_dim 33", (33, (192, 128), 9, True), (33, (192, 128), 1)),
    ("hidden[0] no multiple of 64", (5, (96, 128), 9, True), (5, (192, 128), 1)),
    ("hidden[0] 576", (5, (576, 128), 9, True), (5, (192, 128), 1)),
    ("a later layer 192 wide", (5, (192, 192), 9, True), (5, (192, 128), 1)),
    ("out_dim 33", (5, (192, 128), 33, True), (5, (192, 128), 1)),
    ("a critic outside the envelope", (5, (192, 128), 9, True), (5, (192, 128, 64), 1)),
    ("two observation widths", (5, (192, 128), 9, True), (6, (192, 128), 1)),
    ("a policy without logstd", (5, (192, 128), 9, False), (5, (192, 128), 1)),
    ("a critic with two outputs", (5, (192, 128), 9, True), (5, (192, 128), 2)),
]


def test_refusals_leave_the_key_and_the_outputs_alone(ctx, dev):
    c = rc.Case("three_valu")          # its buffers are large enough for every descriptor below: nothing may be launched anyway
    d = Device(c, dev, c.env())
    ctx.rollout_end()
    obs0, step0 = d.obs_a.clone(), d.ep_step.clone()

    def refused(rc_want, *a, **kw):
        key = (ctypes.c_uint32 * 2)(int(c.key[0]), int(c.key[1]))
        assert _raw_step(ctx, d, *a, key, **kw) == rc_want, (a, kw)
        assert (key[0], key[1]) == (int(c.key[0]), int(c.key[1]))
    for what, p, q in UNSUPPORTED:
        assert not rc.step_supported(*p, *q), what
        refused(RLX_EUNSUP, mlp_desc(p[0], p[1], p[2], nets.ACT_ELU, True, p[3]), mlp_desc(q[0], q[1], q[2], nets.ACT_ELU, True, False))
    refused(RLX_EINVAL, c.pd, c.cd, clip=True)                                    # clip_and_rescale without bounds
    refused(RLX_EINVAL, c.pd, c.cd, clip=True, lo=d.lo)
    refused(RLX_EINVAL, c.pd, c.cd, n_global=c.N - 1)
    refused(RLX_EINVAL, c.pd, c.cd, final_obs=None)                               # fuse_env with a missing env pointer
    torch.cuda.synchronize()
    for k, v in d.full.items():
        if k not in ("obs_a", "ep_step", "ep_ret", "last_ret", "last_len"):
            assert bool((v == SENT).all()), k                                     # nothing was launched
    assert torch.equal(d.obs_a, obs0) and torch.equal(d.ep_step, step0) and d.stats.abs().sum().item() == 0
    # and the accepted call right behind them works
    key = (ctypes.c_uint32 * 2)(int(c.key[0]), int(c.key[1]))
    assert _raw_step(ctx, d, c.pd, c.cd, key, clip=True, lo=d.lo, hi=d.hi) == 0
    assert np.array_equal(np.array([key[0], key[1]], np.uint32), prng.split(c.key, 2, True)[0])
    assert bool(torch.isfinite(d.action).all())
