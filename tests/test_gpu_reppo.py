"""GPU: REPPO's kernels and steps (reppo.hip) against the float64 twin (tests/reppo_twin.py): the RMSNorm trunks through acting and
evaluate_next, the soft TD-lambda scan, REPPO's observation normaliser, one critic step and one policy step (both branches of the
KL `where`, gradient clipping on and off, terminations and truncations), and the whole-update call against the same sequence of
single steps.  Tolerances: 1e-5 relative (L2 per vector), scalars 1e-5."""
import os

import numpy as np
import pytest
import torch

import reppo_twin as tw
from reppo_cases import HP, Case, _close, _f32, _hp, _rel, _t, _with_noise, place_kl_bound, value_floor
from rlx_amd.hip import reppo_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu


def test_param_counts_match_the_twin(ctx):
    c = Case(0, 8)
    assert ctx.reppo_param_count(c.desc, 0) == c.LP["n"] == c.p.size
    assert ctx.reppo_param_count(c.desc, 1) == c.LQ["n"] == c.q.size


@pytest.mark.parametrize("N,H", [(300, 64), (4096, 256)])
def test_act_and_evaluate_next_match_the_twin(ctx, dev, N, H):
    c = Case(1, N, Hp=H, Hc=H, NB=51)
    hp = _hp(c.h)
    obs = c.states
    low, high = np.array([-1.0, -2.0, 0.0]), np.array([1.0, 0.5, 3.0])
    P, Q = _t(c.p, dev), _t(c.q, dev)
    pidx, cidx = _t(c.pidx, dev, np.int32), _t(c.cidx, dev, np.int32)
    act, proc = torch.empty(N, c.A, device=dev), torch.empty(N, c.A, device=dev)
    eps = _t(c.eps_new[:N], dev)
    key = L.prng_key(5)
    _with_noise(ctx, eps, None, lambda: ctx.reppo_act(c.desc, P, _t(obs, dev), key, act, proc, _t(low, dev), _t(high, dev), hp, pidx=pidx))
    ra, rp = tw.act(c.p, c.LP, obs[:, c.pidx], c.eps_new[:N], c.h, low, high)
    assert _rel(act.cpu().numpy(), ra) < 1e-5 and _rel(proc.cpu().numpy(), rp) < 1e-5
    # deterministic: tanh(loc), key untouched
    assert np.array_equal(ctx.reppo_act(c.desc, P, _t(obs, dev), key, act, proc, _t(low, dev), _t(high, dev), hp, True, pidx=pidx), key)
    assert _rel(act.cpu().numpy(), tw.act(c.p, c.LP, obs[:, c.pidx], None, c.h, low, high, True)[0]) < 1e-5
    # sampled from the key: a fresh draw each call, within the action range
    k1 = ctx.reppo_act(c.desc, P, _t(obs, dev), key, act, proc, _t(low, dev), _t(high, dev), hp, pidx=pidx)
    assert not np.array_equal(k1, key) and torch.isfinite(act).all() and (act.abs() <= 1).all()
    nf, nv, sr = torch.empty(N, H, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    _with_noise(ctx, eps, None, lambda: ctx.reppo_evaluate_next(c.desc, P, Q, _t(obs, dev), _t(c.rewards, dev), key, nf, nv, sr, hp, pidx,
                                                                cidx))
    F, v, s = tw.evaluate_next(c.p, c.LP, c.q, c.LQ, obs[:, c.pidx], obs[:, c.cidx], c.rewards, c.eps_new[:N], c.h)
    assert _rel(nf.cpu().numpy(), F) < 1e-5 and _close(nv.cpu().numpy(), v) and _rel(sr.cpu().numpy(), s) < 1e-5


@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
def test_td_lambda_scan(ctx, dev, lam):
    rng = np.random.default_rng(7)
    T, N, g = 37, 1000, 0.97
    sr, nv = _f32(rng.standard_normal((T, N))), _f32(rng.standard_normal((T, N)) * 5)
    te = (rng.random((T, N)) < 0.05).astype(np.float64)
    tr = ((rng.random((T, N)) < 0.05) & (te == 0)).astype(np.float64)
    out = torch.empty(T, N, device=dev)
    ctx.reppo_td_lambda(*(_t(x, dev) for x in (sr, nv, te, tr)), g, lam, out)
    ref = tw.td_lambda(sr, nv, te, tr, g, lam)
    assert _rel(out.cpu().numpy(), ref) < 1e-5
    if lam == 0.0:      # one-step soft TD target
        assert _rel(ref, sr + g * (tr * nv + (1 - tr) * (1 - te) * nv)) < 1e-12
    if lam == 1.0:      # without dones: the discounted soft return bootstrapped from next_values[T - 1]
        z = np.zeros_like(te)
        ret, acc = tw.td_lambda(sr, nv, z, z, g, 1.0), nv[-1].copy()
        for t in range(T - 1, -1, -1):
            acc = sr[t] + g * acc
        assert _rel(ret[0], acc) < 1e-12


def test_observation_normaliser_float32_count(ctx, dev):
    rng = np.random.default_rng(9)
    N, O = 512, 17
    mean, var, cnt = torch.zeros(O, device=dev), torch.ones(O, device=dev), torch.full((1,), 1e-4, device=dev)
    m, v, c = np.zeros(O, np.float32), np.ones(O, np.float32), np.float32(1e-4)
    for i in range(40):
        x = (rng.standard_normal((N, O)) * (1 + np.arange(O)) + 3.0 + 0.1 * i).astype(np.float32)
        ctx.reppo_obs_norm_update(_t(x, dev), mean, var, cnt)
        m, v, c = tw.obs_norm_update(m, v, c, x)
    assert cnt.item() == c                                    # the float32 count, step for step
    assert _rel(mean.cpu().numpy(), m) < 1e-5 and _rel(var.cpu().numpy(), v) < 1e-5
    out = ctx.reppo_obs_norm_apply(_t(x, dev), mean, var, torch.empty(N, O, device=dev))
    assert _rel(out.cpu().numpy(), (x - m) / np.sqrt(v.astype(np.float64) + 1e-8)) < 1e-5


CASES = {  # name -> Case kwargs
    "inside_kl_bound": dict(seed=11, B=64),
    "mixed_kl": dict(seed=12, B=96, old_seed=99, NB=51),
    "clip_active": dict(seed=13, B=64, max_grad_norm=0.05, nr_kl_samples=16),
    "large": dict(seed=14, B=4096, Hp=256, Hc=256, NB=151, old_seed=98, max_grad_norm=0.5),
}


def _case(name):
    return place_kl_bound(Case(**CASES[name]))


@pytest.mark.parametrize("name", list(CASES))
def test_critic_step_matches_the_twin(ctx, dev, name):
    c = _case(name)
    hp = _hp(c.h)
    Q, qm, qv = _t(c.q, dev), torch.zeros(c.q.size, device=dev), torch.zeros(c.q.size, device=dev)
    met = torch.zeros(5, device=dev)
    rows = np.random.default_rng(3).permutation(c.B).astype(np.int32)
    lr = 3e-4
    for step in (1, 2):       # two steps: the second one sees non-zero Adam moments
        q0 = Q.cpu().numpy()
        ctx.reppo_critic_step(c.desc, Q, qm, qv, c.batch_dev(dev), step, lr, hp, met, rows=_t(rows, dev, np.int32),
                              cidx=_t(c.cidx, dev, np.int32))
        tb = tuple(x[rows] for x in c.batch_twin())
        if step == 1:
            rq, rm, rv, rmet, g = tw.critic_step(q0, np.zeros(c.q.size), np.zeros(c.q.size), step, lr, c.LQ, tb, c.h)
        else:
            rq, rm, rv, rmet, g = tw.critic_step(q0, prev_m, prev_v, step, lr, c.LQ, tb, c.h)
        got = met.cpu().numpy()
        for k in range(5):
            assert abs(got[k] - rmet[k]) <= 1e-5 * max(abs(rmet[k]), 1.0), (k, got, rmet)
        if name == "clip_active":
            assert rmet[4] > hp.max_grad_norm
        # the gradient itself is checked through m at 1e-5; Adam's step m / (sqrt(v) + 1e-8) amplifies the float32 rounding of
        # gradients near 1e-8 (first steps), so the parameter step is held to 2e-4
        assert _rel(Q.cpu().numpy() - q0, _f32(rq) - q0) < 2e-4
        # v: the library's Adam launch forms 1 - b2 from float32 b2 = 0.999 (0.00099998713; torch: the double 1 - 0.999), a uniform
        # 1.3e-5 relative offset of the second moments that the update (sqrt(v)) halves
        assert _rel(qm.cpu().numpy(), rm) < 1e-5 and _rel(qv.cpu().numpy(), rv) < 5e-5
        prev_m, prev_v = qm.cpu().numpy().astype(np.float64), qv.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", list(CASES))
def test_policy_step_matches_the_twin(ctx, dev, name):
    c = _case(name)
    hp = _hp(c.h)
    P, pm, pv = _t(c.p, dev), torch.zeros(c.p.size, device=dev), torch.zeros(c.p.size, device=dev)
    OP, Q = _t(c.old_p, dev), _t(c.q, dev)
    met = torch.zeros(9, device=dev)
    en, eo = _t(c.eps_new, dev), _t(c.eps_old, dev)
    q_before = Q.clone()
    _with_noise(ctx, en, eo, lambda: ctx.reppo_policy_step(c.desc, P, pm, pv, OP, Q, _t(c.states, dev), L.prng_key(1), 1, 3e-4, hp, met,
                                                           pidx=_t(c.pidx, dev, np.int32), cidx=_t(c.cidx, dev, np.int32)))
    rp, rm, rv, rmet, g, kl = tw.policy_step(c.p, np.zeros(c.p.size), np.zeros(c.p.size), c.old_p, c.q, 1, 3e-4, c.LP, c.LQ,
                                             c.states[:, c.pidx], c.states[:, c.cidx], c.eps_new, c.eps_old, c.h)
    assert torch.equal(Q, q_before)                              # the critic is frozen: bit for bit
    inside = kl < c.h["kl_bound"]
    if name in ("inside_kl_bound", "clip_active"):
        assert inside.all()
    else:
        assert 0 < inside.sum() < len(kl)                          # both branches of the where
    got = met.cpu().numpy()
    for k in range(9):
        tol = 1e-5 * max(abs(rmet[k]), 1.0) if k != 4 else 1e-5 * max(abs(rmet[k]), 0.1)
        assert abs(got[k] - rmet[k]) <= tol, (k, got, rmet)
    if name == "clip_active":
        assert rmet[8] > hp.max_grad_norm
    gp = pm.cpu().numpy() / 0.1 * (min(1.0, hp.max_grad_norm / (rmet[8] + 1e-6)) ** -1)   # m_1 = 0.1 x clipped gradient
    # >= 4096 rows: the split-operand weight-gradient engine and float32 atanh over K x B x A KL samples -> 2e-5 there
    assert _rel(gp, g) < (2e-5 if c.B >= 4096 else 1e-5)
    assert abs(g[c.LP["coef"]]) > 0 and abs(g[c.LP["coef"] + 1]) > 0     # both coefficient gradients
    assert _rel(gp[c.LP["coef"]:], g[c.LP["coef"]:]) < 1e-5
    # Adam's first step is ~lr sign(g): where a gradient is ~0 its float32 rounding flips the step, so the step is compared on the
    # entries whose gradient is not negligible (the gradient itself was compared above, every entry)
    sel = np.abs(g) > 1e-3 * np.sqrt(np.mean(g * g))
    assert sel.mean() > 0.9
    assert _rel((P.cpu().numpy() - c.p)[sel], (_f32(rp) - c.p)[sel]) < 2e-4 and _rel(pv.cpu().numpy(), rv) < 5e-5


@pytest.mark.parametrize("envs,steps,mbs,epochs", [(32, 8, 4, 2), (4096, 128, 128, 1)])
def test_whole_update_equals_single_steps(ctx, dev, envs, steps, mbs, epochs):
    """rlx_reppo_update_f32 == the same sequence of critic + policy steps (threefry noise); at the reference's default scale only the
    first minibatch is replayed"""
    batch = envs * steps
    c = Case(21, batch, Hp=64 if envs < 4096 else 256, Hc=64 if envs < 4096 else 256, NB=51 if envs < 4096 else 151, old_seed=97,
             nr_kl_samples=4 if envs < 4096 else 16)
    hp = _hp(c.h)
    rng = np.random.default_rng(0)
    idx = np.arange(batch)
    perm = []
    for _ in range(epochs):
        rng.shuffle(idx)
        perm.append(idx.copy())
    perm = np.stack(perm).astype(np.int32)
    pidx, cidx = _t(c.pidx, dev, np.int32), _t(c.cidx, dev, np.int32)
    bd = c.batch_dev(dev)
    z = lambda n: torch.zeros(n, device=dev)
    state0 = [_t(c.p, dev), z(c.p.size), z(c.p.size), _t(c.q, dev), z(c.q.size), z(c.q.size)]
    OP = _t(c.old_p, dev)
    a = [x.clone() for x in state0]
    met = z(epochs * mbs * 14).view(epochs * mbs, 14)
    key0 = L.prng_key(42)
    key, cnt = ctx.reppo_update(c.desc, a[0], a[1], a[2], OP, a[3], a[4], a[5], bd, _t(perm, dev, np.int32), mbs, key0, 0, 3e-4, hp, met,
                                pidx=pidx, cidx=cidx)
    assert cnt == epochs * mbs and torch.isfinite(met).all()
    b = [x.clone() for x in state0]
    mb = batch // mbs
    n_check = epochs * mbs if envs < 4096 else 1
    k = key0
    ref = z(14)
    for i in range(n_check):
        rows = _t(perm.reshape(-1)[i * mb:(i + 1) * mb], dev, np.int32)
        ctx.reppo_critic_step(c.desc, b[3], b[4], b[5], bd, i + 1, 3e-4, hp, ref[:5], rows=rows, cidx=cidx)
        k = ctx.reppo_policy_step(c.desc, b[0], b[1], b[2], OP, b[3], bd[0], k, i + 1, 3e-4, hp, ref[5:], rows=rows, pidx=pidx, cidx=cidx)
        assert torch.equal(ref, met[i]), i
    if n_check == epochs * mbs:
        assert np.array_equal(k, key)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    else:   # the first minibatch at full size against the twin: critic step, then the policy step on the updated critic with
        # injected noise (the same call again from the initial state; only its first minibatch is compared)
        rows = perm[0, :mb]
        tb = tuple(x[rows] for x in c.batch_twin())
        rq, _, _, rmet, _ = tw.critic_step(c.q, np.zeros(c.q.size), np.zeros(c.q.size), 1, 3e-4, c.LQ, tb, c.h)
        got = met[0, :5].cpu().numpy()
        for j in range(5):
            assert abs(got[j] - rmet[j]) <= 1e-5 * max(abs(rmet[j]), 1.0), (j, got, rmet)
        rng = np.random.default_rng(5)
        en = rng.standard_normal((mb, c.A)).astype(np.float32)
        eo = rng.standard_normal((c.h["nr_kl_samples"], mb, c.A)).astype(np.float32)
        a = [x.clone() for x in state0]
        ten, teo = _t(en, dev), _t(eo, dev)
        _with_noise(ctx, ten, teo, lambda: ctx.reppo_update(c.desc, a[0], a[1], a[2], OP, a[3], a[4], a[5], bd, _t(perm, dev, np.int32), mbs,
                                                            key0, 0, 3e-4, hp, met, pidx=pidx, cidx=cidx))
        s_rows = c.states[rows]
        _, _, _, pmet, _, _ = tw.policy_step(c.p, np.zeros(c.p.size), np.zeros(c.p.size), c.old_p, rq, 1, 3e-4, c.LP, c.LQ,
                                             s_rows[:, c.pidx], s_rows[:, c.cidx], en, eo, c.h)
        got = met[0, 5:].cpu().numpy()
        for j in range(9):
            tol = 1e-5 * max(abs(pmet[j]), 1.0) if j != 4 else 1e-5 * max(abs(pmet[j]), 0.1)
            assert abs(got[j] - pmet[j]) <= tol, (j, got, pmet)
        assert torch.isfinite(met).all()


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_steps_match_the_reference_fixture(ctx, dev, c):
    """one critic step, then one policy step on the updated critic, against the outputs of the reference's own closures"""
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "reppo_reference.npz"))
    k = "c%d_" % c
    g = lambda n: z[k + n]
    fc = tw.fixture_case(z, c)
    O, A, Hp, Hc, NB, B = (fc[n] for n in ("O", "A", "Hp", "Hc", "NB", "B"))
    h, p, q, old_p = dict(HP, **fc["hp"]), fc["p"], fc["q"], fc["old_p"]
    hp = _hp(h)
    desc = reppo_desc(O, O, A, Hp, Hc, NB)
    P, Q, OP = _t(p, dev), _t(q, dev), _t(old_p, dev)
    z_ = lambda n: torch.zeros(n, device=dev)
    pm, pv, qm, qv = z_(p.size), z_(p.size), z_(q.size), z_(q.size)
    batch = tuple(_t(g(n), dev) for n in ("states", "actions", "rewards", "targets", "next_features", "terms", "truncs"))
    nf, nv, sr = torch.empty(B, Hc, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    ee = _t(g("eps_eval"), dev)
    _with_noise(ctx, ee, None, lambda: ctx.reppo_evaluate_next(desc, P, Q, _t(g("next_states"), dev), batch[2], L.prng_key(0), nf, nv, sr, hp))
    assert _rel(nf.cpu().numpy(), g("eval_next_features")) < 1e-5 and _close(nv.cpu().numpy(), g("eval_next_value"), value_floor(h))
    assert _rel(sr.cpu().numpy(), g("eval_soft_reward")) < 1e-5
    cm, pmet = z_(5), z_(9)
    ctx.reppo_critic_step(desc, Q, qm, qv, batch, 1, 3e-4, hp, cm)
    ref = g("critic_metrics")
    got = cm.cpu().numpy()
    for j in range(5):
        assert abs(got[j] - ref[j]) <= 1e-5 * max(abs(ref[j]), 1.0), (j, got, ref)
    q_after = Q.clone()
    en, eo = _t(g("eps_new"), dev), _t(g("eps_old"), dev)
    _with_noise(ctx, en, eo, lambda: ctx.reppo_policy_step(desc, P, pm, pv, OP, Q, batch[0], L.prng_key(1), 1, 3e-4, hp, pmet))
    assert torch.equal(Q, q_after)
    ref = g("policy_metrics")
    got = pmet.cpu().numpy()
    # new_lp_at_old goes through atanh(clamp(tanh(old base))) in float32 as the reference computes it: one float32 ulp of the old
    # action a moves b = atanh(a) by ulp / (1 - a^2), and the log-prob by |d new_lp / d b| <= |u| / std + 2 times that.  The
    # fixture's bases reach |3.6| .. |6.5|, where this conditioning exceeds 1e-5 of the KL: the KL-dependent scalars (clipped loss,
    # kl coefficient loss, kl) get that float32 bound on top of the 1e-5 bar.
    with torch.no_grad():
        LP, LQ = fc["LP"], fc["LQ"]
        oloc, ols = tw.policy_fwd(torch.tensor(old_p, dtype=torch.float64), LP, torch.tensor(g("states")))
        loc, ls = tw.policy_fwd(torch.tensor(p, dtype=torch.float64), LP, torch.tensor(g("states")))
        oa = torch.tanh(oloc + (ols.exp() + h["policy_min_std"]) * torch.tensor(g("eps_old")))
        b = torch.atanh(torch.clamp(oa, -1 + 1e-6, 1 - 1e-6))
        std = ls.exp() + h["policy_min_std"]
        sens = ((b - loc) / std).abs() / std + 2.0
        kl_f32 = float(((2.0 ** -24) / (1.0 - oa * oa) * sens).sum(-1).mean())
    beta = float(np.exp(p[LP["coef"] + 1]))
    for j in range(9):
        tol = 1e-5 * max(abs(ref[j]), 1.0) if j != 4 else 1e-5 * max(abs(ref[j]), 0.1)
        tol += {0: beta * kl_f32, 2: beta * kl_f32, 4: kl_f32}.get(j, 0.0)
        assert abs(got[j] - ref[j]) <= tol, (j, got, ref, kl_f32)
    # the clipped gradients (m_1 = 0.1 x clipped gradient): the critic's at the fixture's sampled positions; the policy's against
    # the twin with the old actions rounded to float32 before atanh (the reference's float32 arithmetic; the exact-twin-vs-fixture
    # agreement is pinned at 1e-12 on the CPU, tests/test_reppo_twin.py)
    idx = z[k + "gcritic_idx"]
    assert _rel(qm.cpu().numpy()[idx] / 0.1, z[k + "gcritic_val"]) < 1e-5
    zq = np.zeros(q.size)
    rq = tw.critic_step(q, zq, zq, 1, 3e-4, LQ, tuple(g(n) for n in ("states", "actions", "targets", "rewards", "next_features", "terms", "truncs")),
                        h)[0]
    _, _, _, rmet, gp, _ = tw.policy_step(p, np.zeros(p.size), np.zeros(p.size), old_p, rq, 1, 3e-4, LP, LQ,
                                          g("states"), g("states"), g("eps_new"), g("eps_old"), h, f32_old_action=True)
    gp_clipped = gp * min(1.0, h["max_grad_norm"] / (rmet[8] + 1e-6))
    assert _rel(pm.cpu().numpy() / 0.1, gp_clipped) < 1e-5


def _reppo_plugin(env_over, alg_over, pidx=None, cidx=None):
    import rlx_amd.algorithms.reppo.hip  # noqa: F401
    from test_gpu_obs_indices import _plugin
    return _plugin("reppo.hip", env_over, alg_over, pidx, cidx)


@pytest.mark.parametrize("indices", [False, True])
def test_plugin_trains_on_the_synthetic_env(dev, tmp_path, indices):
    """A few iterations of `reppo.hip` end to end: rollout, targets, whole update, metrics, evaluation, checkpoint round trip."""
    from rlx_amd.algorithms.reppo.hip.reppo import METRIC_NAMES
    pidx, cidx = (np.arange(0, 10), np.arange(6, 24)) if indices else (None, None)
    cls, config, env = _reppo_plugin(dict(nr_envs=32, obs_dim=24, act_dim=4, horizon=12),
                                     dict(nr_steps=8, nr_epochs=2, nr_minibatches=4, policy_hidden_dim=64, critic_hidden_dim=64, nr_bins=51,
                                          nr_kl_samples=4, total_timesteps=3 * 32 * 8, evaluation_frequency=32 * 8, evaluation_episodes=4,
                                          anneal_learning_rate=True), pidx, cidx)
    config.runner.save_model = True
    m = cls(config, env, env, str(tmp_path), None)
    assert (m.desc.policy_obs_dim, m.desc.critic_obs_dim) == ((10, 18) if indices else (24, 24))
    p0, q0 = m.pparams.clone(), m.qparams.clone()
    m.train()
    assert all(np.isfinite(v) for v in m.last_metrics.values()), m.last_metrics
    for k in METRIC_NAMES + ("lr/learning_rate", "eval/episode_return"):
        assert k in m.last_metrics, k
    assert m.opt_count == 3 * 2 * 4 and m.nr_iterations_done == 3
    assert (m.pparams - p0).abs().max().item() > 0 and (m.qparams - q0).abs().max().item() > 0
    L_ = __import__("reppo_twin").policy_layout(m.desc.policy_obs_dim, 4, 64)
    assert (m.pparams[L_["coef"]:] - p0[L_["coef"]:]).abs().min().item() > 0      # both log-coefficients moved
    assert abs(m.last_metrics["lr/learning_rate"]) < 1e-12          # LinearLR annealed to 0 after the last iteration
    cnt = np.float32(1e-4)
    for _ in range(3 * 8):
        cnt = np.float32(cnt + np.float32(32))
    assert float(m.norm_count.item()) == cnt                          # one float32 update per rollout step
    path = os.path.join(str(tmp_path), "models", "best.model")
    m.save()
    config.runner.load_model = path
    m2 = cls.load(config, env, env, str(tmp_path), None, [])
    for k in cls._STATE:
        assert torch.equal(getattr(m2, k), getattr(m, k)), k
    assert m2.opt_count == m.opt_count
    assert len(m2.test(3)) == 3


def test_runner_trains_and_tests_reppo_from_the_command_line(monkeypatch, tmp_path):
    import sys
    from rlx_amd.runner.runner import Runner
    monkeypatch.chdir(tmp_path)
    base = ["experiment.py", "--algorithm.name=reppo.hip", "--environment.name=synthetic.random_obs", "--environment.nr_envs=32",
            "--environment.obs_dim=20", "--environment.act_dim=3", "--environment.horizon=6"]
    flags = ["--algorithm.nr_steps=4", "--algorithm.nr_minibatches=2", "--algorithm.nr_epochs=1", "--algorithm.policy_hidden_dim=64",
             "--algorithm.critic_hidden_dim=64", "--algorithm.total_timesteps=256"]
    monkeypatch.setattr(sys, "argv", base + ["--runner.mode=train", "--runner.save_model=true", "--runner.run_name=reppo"] + flags)
    trained = Runner().run()
    path = os.path.join(trained.save_path, "best.model")
    assert os.path.exists(path) and trained.opt_count == 2 * 2
    monkeypatch.setattr(sys, "argv", base + ["--runner.mode=test", f"--runner.load_model={path}", "--runner.nr_test_episodes=2"])
    tested = Runner().run()
    ckpt = np.load(path, allow_pickle=False)
    assert torch.equal(tested.pparams.cpu(), torch.from_numpy(ckpt["pparams"])) and tested.opt_count == int(ckpt["opt_count"]) > 0
