"""GPU: FastTD3's networks and update steps (fasttd3.hip) against the reference's own outputs (tests/golden/fasttd3_reference.npz)
and against the float64 twin (tests/fasttd3_twin.py) at the reference's default batch; noise scales, acting, the two-stream
schedule, and the `fasttd3.hip` plugin end to end.  Tolerances: 1e-5 relative (L2 per vector), scalars 1e-5."""
import os

import numpy as np
import pytest
import torch

import fasttd3_twin as tw
from oracle import prng
from fasttd3_cases import KINK_TAU, MAX_FLIPS, _explain, _fwd_flip, _hp, _kinks, _rel, _t
from rlx_amd.hip import relu_mlp_desc
from test_fasttd3_twin import check_sampled, fixture_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", [0, 1, 2])
def test_acting_matches_the_reference_policy(ctx, dev, c):
    z, g, h, O, A, NA, B, pflat, qflat, clipped = fixture_case(c)
    from rlx_amd.hip import lib as L
    pd = relu_mlp_desc(O, tw.POLICY_HIDDEN, A)
    assert ctx.lib.rlx_mlp_param_count(pd) == pflat.size
    P, s = _t(pflat, dev), _t(g("states"), dev)
    act, proc = torch.empty(B, A, device=dev), torch.empty(B, A, device=dev)
    key = L.prng_key(3)
    assert np.array_equal(ctx.fasttd3_act(pd, P, s, None, key, act, proc, deterministic=True), key)     # no draw: key untouched
    assert _rel(act.cpu().numpy(), g("deterministic_action")) < 1e-5 and torch.equal(act, proc)
    clip = bool(int(g("clip_and_rescale")))
    low, high = (_t(g("low"), dev), _t(g("high"), dev)) if clip else (None, None)
    eps = _t(g("act_noise"), dev)              # (the library keeps the pointer: the tensor must outlive the call)
    ctx.dbg_set_sac_noise(eps, None)
    try:
        ctx.fasttd3_act(pd, P, s, _t(g("noise_scales"), dev), key, act, proc, low=low, high=high)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    assert _rel(act.cpu().numpy(), g("action")) < 1e-5 and _rel(proc.cpu().numpy(), g("processed_action")) < 1e-5
    # with clip-and-rescale the ring's action is the UNclipped one: it leaves [-1, 1] where the env's does not
    if clip:
        assert np.all(proc.cpu().numpy() >= g("low") - 1e-6) and np.all(proc.cpu().numpy() <= g("high") + 1e-6)


def test_act_clip_and_rescale_on_and_off(ctx, dev):
    from rlx_amd.hip import lib as L
    rng = np.random.default_rng(4)
    O, A, N = 17, 5, 300
    pflat, _ = tw.make_params(9, O, A, 11)
    pd = relu_mlp_desc(O, tw.POLICY_HIDDEN, A)
    obs = rng.standard_normal((N, O)).astype(np.float32)
    eps = (3.0 * rng.standard_normal((N, A))).astype(np.float32)                  # large draws: many actions beyond [-1, 1]
    scales = rng.uniform(0.1, 0.9, N).astype(np.float32)
    low, high = np.linspace(-2.0, -0.5, A).astype(np.float32), np.linspace(0.5, 3.0, A).astype(np.float32)
    out = {}
    eps_d = _t(eps, dev)
    ctx.dbg_set_sac_noise(eps_d, None)
    try:
        for clip in (False, True):
            act, proc = torch.empty(N, A, device=dev), torch.empty(N, A, device=dev)
            ctx.fasttd3_act(pd, _t(pflat, dev), _t(obs, dev), _t(scales, dev), L.prng_key(1), act, proc,
                            low=_t(low, dev) if clip else None, high=_t(high, dev) if clip else None)
            out[clip] = (act.cpu().numpy(), proc.cpu().numpy())
    finally:
        ctx.dbg_set_sac_noise(None, None)
    for clip in (False, True):
        ea, ep = tw.act(pflat, O, A, obs, eps, scales, low if clip else None, high if clip else None)
        assert _rel(out[clip][0], ea) < 1e-5 and _rel(out[clip][1], ep) < 1e-5
    assert np.array_equal(out[False][0], out[True][0]) and np.array_equal(out[False][0], out[False][1])
    assert (np.abs(out[True][0]) > 1).any() and np.all(out[True][1] >= low) and np.all(out[True][1] <= high)


def test_noise_scales_redraw(ctx, dev):
    from rlx_amd.hip import lib as L
    N, lo, hi = 5000, 0.001, 0.4
    s = torch.empty(N, device=dev)
    key0 = L.prng_key(8)
    key1 = ctx.fasttd3_noise_scales(key0, s, lo, hi)
    first = s.cpu().numpy()
    assert first.min() >= lo and first.max() < hi and first.std() > 0.05
    # reproducible from the key: u_i = uniform(bits(subkey, i of N)) of the counter RNG
    sub = prng.split(key0, 2)[1]
    exp = np.float32(prng.uniform(sub, (N,))) * np.float32(hi - lo) + np.float32(lo)
    np.testing.assert_allclose(first, exp, rtol=1e-6)
    assert np.array_equal(key1, prng.split(key0, 2)[0])
    dones = (np.random.default_rng(0).random(N) < 0.1).astype(np.float32)
    key2 = ctx.fasttd3_noise_scales(key1, s, lo, hi, dones=_t(dones, dev))
    second = s.cpu().numpy()
    assert np.array_equal(second[dones == 0], first[dones == 0])
    assert np.all(second[dones > 0] != first[dones > 0]) and second.min() >= lo and second.max() < hi
    s2 = torch.empty(N, device=dev)
    ctx.fasttd3_noise_scales(key0, s2, lo, hi)
    assert torch.equal(s2.cpu(), torch.from_numpy(first)) and not np.array_equal(key2, key1)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_critic_and_policy_steps_match_the_reference_closures(ctx, dev, c):
    z, g, h, O, A, NA, B, pflat, qflat, clipped = fixture_case(c)
    from rlx_amd.hip import lib as L
    pd, qd = relu_mlp_desc(O, tw.POLICY_HIDDEN, A), relu_mlp_desc(O + A, tw.CRITIC_HIDDEN, NA)
    hp = _hp(h, NA, clipped)
    P, Q, QT = _t(pflat, dev), _t(np.concatenate(qflat[:2]), dev), _t(np.concatenate(qflat[2:]), dev)
    zl = torch.zeros_like
    qm, qv, pm, pv = zl(Q), zl(Q), zl(P), zl(P)
    met, pmet = torch.zeros(4, device=dev), torch.zeros(2, device=dev)
    batch = tuple(_t(g(n), dev) for n in ("states", "next_states", "actions", "rewards", "dones", "truncations", "n_steps"))
    eps = _t(g("noise_next"), dev)
    ctx.dbg_set_sac_noise(eps, None)
    try:
        key, cnt = ctx.fasttd3_critic_update(pd, P, qd, Q, qm, qv, QT, batch, L.prng_key(5), 0, hp, met)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    assert cnt == 1
    m = met.cpu().numpy().astype(np.float64)
    for i, name in enumerate(("q_loss", "q_min", "q_max", "critic_grad_norm")):
        assert m[i] == pytest.approx(float(g(name)), rel=1e-5, abs=1e-6), name
    # first AdamW step from zero moments: m = (1 - b1) g, g the gradient after clip_grad_norm_ (what the fixture holds)
    check_sampled(z, "c%d_gcritic" % c, qm.cpu().numpy().astype(np.float64) / 0.1, 1e-5)
    check_sampled(z, "c%d_qparams_after" % c, Q.cpu().numpy(), 1e-5)
    check_sampled(z, "c%d_qtarget_after" % c, QT.cpu().numpy(), 1e-5)
    cnt = ctx.fasttd3_policy_update(pd, P, pm, pv, qd, Q, batch[0], 0, hp, pmet)
    assert cnt == 1
    pmv = pmet.cpu().numpy().astype(np.float64)
    assert pmv[0] == pytest.approx(float(g("policy_loss")), rel=1e-5, abs=1e-6)
    assert pmv[1] == pytest.approx(float(g("policy_grad_norm")), rel=1e-5)
    check_sampled(z, "c%d_gpolicy" % c, pm.cpu().numpy().astype(np.float64) / 0.1, 1e-5)
    check_sampled(z, "c%d_pparams_after" % c, P.cpu().numpy(), 1e-5)


@pytest.mark.parametrize("clipped", [True, False])
def test_steps_at_the_default_batch_against_the_float64_twin(ctx, dev, clipped):
    """B = 32768 with the reference's 1024-512-256 critics (fasttd3/pytorch/default_config.py, q_network.py), obs 48 / act 12,
    nr_atoms 101: every trunk GEMM on the split-operand engine, in both steps.  The 1e-5 bar is defined where the fp32 gradient
    is: a ReLU unit-sample whose float64 pre-activation lies within fp32 rounding of zero (KINK_TAU of its row's RMS), and with
    clipped double Q a row whose two expectations agree to within their fp32 error, may come out on either side in ANY fp32
    evaluation, and that sample's whole contribution through the unit / the chosen critic flips with it.  The candidates are
    counted from float64 alone; for each, the twin's gradient with that one unit-sample / row choice inverted is the admissible
    alternative (_explain).  The device has to agree to 1e-5 with the twin for an assignment of at most MAX_FLIPS of them per
    update step."""
    from rlx_amd.hip import lib as L
    rng = np.random.default_rng(12 if clipped else 13)
    O, A, NA, B = 48, 12, 101, 32768
    h = dict(gamma=0.97, tau=0.1, v_min=-10.0, v_max=10.0, learning_rate=3e-4, weight_decay=0.1, smoothing_epsilon=0.2,
             smoothing_clip_value=0.5, max_grad_norm=-1.0)
    pflat, qflat = tw.make_params(41, O, A, NA)
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    s, s2 = f32(rng.standard_normal((B, O))), f32(rng.standard_normal((B, O)))
    a = f32(np.clip(0.6 * rng.standard_normal((B, A)), -1, 1))
    rew, done = f32(3.0 * rng.standard_normal(B)), f32(rng.random(B) < 0.2)
    trunc, nst = f32((rng.random(B) < 0.5) * done), f32(rng.integers(1, 4, B))
    eps = f32(rng.standard_normal((B, A)))
    batch64 = tuple(np.asarray(x, dtype=np.float64) for x in (s, s2, a, rew, done, trunc, nst))
    q64 = [q.astype(np.float64) for q in qflat]
    r = tw.critic_step(pflat.astype(np.float64), *q64, O, A, NA, batch64, eps, h, clipped)
    pd, qd = relu_mlp_desc(O, tw.POLICY_HIDDEN, A), relu_mlp_desc(O + A, tw.CRITIC_HIDDEN, NA)
    hp = _hp(h, NA, clipped)
    P, Q, QT = _t(pflat, dev), _t(np.concatenate(qflat[:2]), dev), _t(np.concatenate(qflat[2:]), dev)
    zl = torch.zeros_like
    qm, qv, pm, pv = zl(Q), zl(Q), zl(P), zl(P)
    met, pmet = torch.zeros(4, device=dev), torch.zeros(2, device=dev)
    batch = tuple(_t(x, dev) for x in (s, s2, a, rew, done, trunc, nst))
    eps_d = _t(eps, dev)
    ctx.dbg_set_sac_noise(eps_d, None)
    try:
        ctx.prof_begin()
        key, cnt = ctx.fasttd3_critic_update(pd, P, qd, Q, qm, qv, QT, batch, L.prng_key(5), 0, hp, met)
        ctx.prof_end()
    finally:
        ctx.dbg_set_sac_noise(None, None)
    gemm = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    assert gemm and not any(q["engine"] == 0 for q in gemm), [q for q in gemm if q["engine"] == 0]   # no silent exact-fp32 fallback
    m = met.cpu().numpy().astype(np.float64)
    exp = [r["q_loss"], r["q_min"], r["q_max"], np.linalg.norm(np.concatenate([r["g_q1"], r["g_q2"]]))]
    for i in range(4):
        assert m[i] == pytest.approx(exp[i], rel=1e-5), (i, m[i], exp[i])
    n = qflat[0].size
    T = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))
    x = np.concatenate([s, a], 1).astype(np.float64)
    tgt = [r["target1"], r["target2"]]

    def critic_row_grad(k, row, flips, t_row):
        Qk = T(q64[k]).requires_grad_(True)
        lg = _fwd_flip(Qk, O + A, tw.CRITIC_HIDDEN, NA, T(x[row:row + 1]), flips)
        (-(T(t_row) * torch.log_softmax(lg, dim=1)).sum() / B).backward()
        return Qk.grad.numpy()
    gq_d = qm.cpu().numpy().astype(np.float64) / 0.1
    ge = np.concatenate([r["g_q1"], r["g_q2"]])
    cands = [(c[0], "relu", k) + c[1:] for k in range(2) for c in _kinks(q64[k], O + A, tw.CRITIC_HIDDEN, x, KINK_TAU)]
    if clipped:                     # rows whose projections' expectations tie: either projection is the target of both critics
        tie = np.abs(r["v1"] - r["v2"]) / np.sqrt(0.5 * (r["v1"] ** 2 + r["v2"] ** 2).mean())
        cands += [(float(tie[i]), "tie", -1, int(i)) for i in np.nonzero(tie < KINK_TAU)[0]]

    def delta(c):
        d = np.zeros_like(ge)
        if c[1] == "relu":
            _, _, k, row, li, j = c
            d[k * n:(k + 1) * n] = critic_row_grad(k, row, {(li, j)}, tgt[k][row:row + 1]) - critic_row_grad(k, row, set(), tgt[k][row:row + 1])
        else:
            row = c[3]
            other = r["p2"][row:row + 1] if r["v1"][row] < r["v2"][row] else r["p1"][row:row + 1]
            for k in range(2):
                d[k * n:(k + 1) * n] = critic_row_grad(k, row, set(), other) - critic_row_grad(k, row, set(), tgt[k][row:row + 1])
        return d
    ga, taken = _explain(gq_d, ge, cands, delta, MAX_FLIPS)
    print(f"FastTD3 critic step at B={B}: ||dg||/||g|| = {_rel(gq_d, ge):.2e}, {_rel(gq_d, ga):.2e} with {len(taken)} of the "
          f"{len(cands)} kink / tie candidates on their other side: {[c[1:] for c in taken]}")
    assert _rel(gq_d, ga) < 1e-5 and len(taken) <= MAX_FLIPS
    # policy step on the device's updated critics; the twin gets exactly those parameters
    qa = Q.cpu().numpy().astype(np.float64)
    qn = [qa[:n], qa[n:]]
    p = tw.policy_step(pflat.astype(np.float64), qn[0], qn[1], O, A, NA, s.astype(np.float64), h, clipped)
    ctx.prof_begin()
    cnt = ctx.fasttd3_policy_update(pd, P, pm, pv, qd, Q, batch[0], 0, hp, pmet)
    ctx.prof_end()
    gemm = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    assert gemm and not any(q["engine"] == 0 for q in gemm), [q for q in gemm if q["engine"] == 0]   # no silent exact-fp32 fallback
    pmv = pmet.cpu().numpy().astype(np.float64)
    assert pmv[0] == pytest.approx(p["policy_loss"], rel=1e-5, abs=1e-6)
    assert pmv[1] == pytest.approx(np.linalg.norm(p["g_policy"]), rel=1e-5)
    gp_d = pm.cpu().numpy().astype(np.float64) / 0.1
    z = T(np.linspace(h["v_min"], h["v_max"], NA))

    def policy_row_grad(row, flips, swap_min):
        Pp = T(pflat).requires_grad_(True)
        act_ = torch.tanh(_fwd_flip(Pp, O, tw.POLICY_HIDDEN, A, T(s[row:row + 1]), flips.get("pi", set())))
        xa = torch.cat([T(s[row:row + 1]), act_], dim=1)
        v = [(torch.softmax(_fwd_flip(T(qn[k]), O + A, tw.CRITIC_HIDDEN, NA, xa, flips.get(k, set())), dim=1) * z).sum() for k in range(2)]
        if clipped:
            first = bool(v[0] < v[1]) != swap_min
            q = v[0] if first else v[1]
        else:
            q = 0.5 * (v[0] + v[1])
        (-q / B).backward()
        return Pp.grad.numpy()
    xp = np.concatenate([s, p["actions"]], 1)
    pc = [(c[0], "relu", "pi") + c[1:] for c in _kinks(pflat.astype(np.float64), O, tw.POLICY_HIDDEN, s, KINK_TAU)]
    pc += [(c[0], "relu", k) + c[1:] for k in range(2) for c in _kinks(qn[k], O + A, tw.CRITIC_HIDDEN, xp, KINK_TAU)]
    if clipped:
        vv = np.stack([(np.exp(lg - lg.max(1, keepdims=True)) / np.exp(lg - lg.max(1, keepdims=True)).sum(1, keepdims=True)) @ z.numpy()
                       for lg in (tw.critic_logits(T(qn[k]), O, A, NA, T(s), T(p["actions"])).numpy() for k in range(2))])
        tie = np.abs(vv[0] - vv[1]) / np.sqrt(0.5 * (vv ** 2).sum(0).mean())
        pc += [(float(tie[i]), "min", -1, int(i)) for i in np.nonzero(tie < KINK_TAU)[0]]

    def pdelta(c):
        row = c[3]
        if c[1] == "min":
            return policy_row_grad(row, {}, True) - policy_row_grad(row, {}, False)
        return policy_row_grad(row, {c[2]: {(c[4], c[5])}}, False) - policy_row_grad(row, {}, False)
    gpa, ptaken = _explain(gp_d, p["g_policy"], pc, pdelta, MAX_FLIPS)
    print(f"FastTD3 policy step at B={B}: ||dg||/||g|| = {_rel(gp_d, p['g_policy']):.2e}, {_rel(gp_d, gpa):.2e} with {len(ptaken)} of "
          f"the {len(pc)} kink / tie candidates on their other side: {[c[1:] for c in ptaken]}")
    assert _rel(gp_d, gpa) < 1e-5 and len(ptaken) <= MAX_FLIPS


def test_two_stream_schedule_is_bit_identical_to_one_stream(ctx, dev):
    from rlx_amd.hip import lib as L
    rng = np.random.default_rng(7)
    O, A, NA, B = 48, 12, 101, 8192
    h = dict(gamma=0.97, tau=0.1, v_min=-10.0, v_max=10.0, learning_rate=3e-4, weight_decay=0.1, smoothing_epsilon=0.001,
             smoothing_clip_value=0.5, max_grad_norm=-1.0)
    pflat, qflat = tw.make_params(43, O, A, NA)
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    s, s2 = f32(rng.standard_normal((B, O))), f32(rng.standard_normal((B, O)))
    a = f32(np.clip(0.6 * rng.standard_normal((B, A)), -1, 1))
    rew, done = f32(3.0 * rng.standard_normal(B)), f32(rng.random(B) < 0.2)
    trunc, nst = f32((rng.random(B) < 0.5) * done), f32(rng.integers(1, 4, B))
    pd, qd = relu_mlp_desc(O, tw.POLICY_HIDDEN, A), relu_mlp_desc(O + A, tw.CRITIC_HIDDEN, NA)
    hp = _hp(h, NA, True)
    batch = tuple(_t(x, dev) for x in (s, s2, a, rew, done, trunc, nst))

    def run(two):
        ctx.set_option("two_streams", two)
        P, Q, QT = _t(pflat, dev), _t(np.concatenate(qflat[:2]), dev), _t(np.concatenate(qflat[2:]), dev)
        zl = torch.zeros_like
        qm, qv, pm, pv = zl(Q), zl(Q), zl(P), zl(P)
        met, pmet = torch.zeros(4, device=dev), torch.zeros(2, device=dev)
        key, cnt, pcnt = L.prng_key(11), 0, 0
        for _ in range(3):
            key, cnt = ctx.fasttd3_critic_update(pd, P, qd, Q, qm, qv, QT, batch, key, cnt, hp, met)
            pcnt = ctx.fasttd3_policy_update(pd, P, pm, pv, qd, Q, batch[0], pcnt, hp, pmet)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (P, Q, QT, qm, qv, pm, pv, met, pmet)]
    try:
        one, two = run(0), run(1)
    finally:
        ctx.set_option("two_streams", 1)
    for x, y, name in zip(one, two, ("policy", "critics", "targets", "qm", "qv", "pm", "pv", "critic metrics", "policy metrics")):
        assert np.isfinite(x).all() and np.array_equal(x, y), name


def _fasttd3_plugin(env_over, alg_over, pidx=None, cidx=None):
    import rlx_amd.algorithms.fasttd3.hip  # noqa: F401
    from test_gpu_obs_indices import _plugin
    return _plugin("fasttd3.hip", env_over, alg_over, pidx, cidx)


@pytest.mark.parametrize("n_steps,indices", [(1, False), (3, False), (1, True)])
def test_plugin_trains_on_the_synthetic_env(dev, tmp_path, n_steps, indices):
    """A few vector steps of `fasttd3.hip` end to end: noise scales, acting, the ring, n-step sampling, normaliser, 2 x 2 critic /
    policy cadence, logging, evaluation, checkpoint round trip."""
    pidx, cidx = (np.arange(0, 10), np.arange(6, 24)) if indices else (None, None)
    cls, config, env = _fasttd3_plugin(dict(nr_envs=32, obs_dim=24, act_dim=4, horizon=12),
                                       dict(batch_size=64, buffer_size_per_env=8, learning_starts=3, n_steps=n_steps, nr_atoms=51,
                                            nr_critic_updates_per_policy_update=2, nr_policy_updates_per_step=2,
                                            total_timesteps=32 * 12, logging_frequency=32 * 4, evaluation_frequency=32 * 8,
                                            save_frequency=32 * 4, action_clipping_and_rescaling=indices), pidx, cidx)
    config.runner.save_model = True
    m = cls(config, env, env, str(tmp_path), None)
    assert (m.pdesc.in_dim, m.qdesc.in_dim, m.qdesc.out_dim) == ((10, 18 + 4, 51) if indices else (24, 28, 51))
    p0, q0, t0 = m.pparams.clone(), m.qparams.clone(), m.qtarget.clone()
    m.train()
    assert all(np.isfinite(v) for v in m.last_metrics.values()), m.last_metrics
    for k in ("loss/q_loss", "loss/policy_loss", "q/q_min", "q/q_max", "gradients/critic_grad_norm", "gradients/policy_grad_norm",
              "lr/learning_rate"):
        assert k in m.last_metrics, k
    assert m.critic_count == 9 * 4 and m.policy_count == 9 * 2          # steps 4..12 optimise: 2 x 2 critic, 2 policy updates each
    assert (m.pparams - p0).abs().max().item() > 0 and (m.qparams - q0).abs().max().item() > 0 and (m.qtarget - t0).abs().max().item() > 0
    ns = m.noise_scales.cpu().numpy()
    assert ns.min() >= 0.001 and ns.max() < 0.4
    assert m.size == 8 and m.pos == 12 % 8
    if m.obs_norm:
        assert int(m.norm_count[0]) == 9 * 2 * 4 * 64
    assert "eval/episode_return" in m.last_metrics
    path = os.path.join(str(tmp_path), "models", "latest.model")
    assert os.path.exists(path)
    config.runner.load_model = path
    m2 = cls.load(config, env, env, str(tmp_path), None, [])
    m.save()
    m3 = cls.load(config, env, env, str(tmp_path), None, [])
    for k in cls._STATE:
        assert torch.equal(getattr(m3, k), getattr(m, k)), k
    assert m2.critic_count > 0 and m3.critic_count == m.critic_count
    assert len(m3.test(2)) <= 2


def test_runner_trains_and_tests_fasttd3_from_the_command_line(monkeypatch, tmp_path):
    import sys
    from rlx_amd.runner.runner import Runner
    monkeypatch.chdir(tmp_path)
    base = ["experiment.py", "--algorithm.name=fasttd3.hip", "--environment.name=synthetic.random_obs", "--environment.nr_envs=32",
            "--environment.obs_dim=20", "--environment.act_dim=3", "--environment.horizon=6"]
    flags = ["--algorithm.batch_size=64", "--algorithm.buffer_size_per_env=8", "--algorithm.learning_starts=2", "--algorithm.nr_atoms=31",
             "--algorithm.total_timesteps=320", "--algorithm.logging_frequency=64", "--algorithm.save_frequency=64"]
    monkeypatch.setattr(sys, "argv", base + ["--runner.mode=train", "--runner.save_model=true", "--runner.run_name=ftd3"] + flags)
    trained = Runner().run()
    path = os.path.join(trained.save_path, "latest.model")
    assert os.path.exists(path) and trained.critic_count == 8 * 2 and trained.policy_count == 8 * 1
    monkeypatch.setattr(sys, "argv", base + ["--runner.mode=test", f"--runner.load_model={path}", "--runner.nr_test_episodes=2"])
    tested = Runner().run()
    ckpt = np.load(path, allow_pickle=False)
    assert torch.equal(tested.pparams.cpu(), torch.from_numpy(ckpt["pparams"])) and tested.critic_count == int(ckpt["critic_count"]) > 0
