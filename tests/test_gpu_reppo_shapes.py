"""GPU: REPPO (reppo.hip) across the shape envelope rlx_reppo_desc / rlx_reppo_hparams accept, against the float64 twin
(tests/reppo_twin.py), at the bars of test_gpu_reppo.py (tests/reppo_cases.py).

Critic step (two, so the second sees non-zero Adam moments) and policy step per case, injected noise.  The paths each case is
there for, worked out from the host selection code (fs_head_bwd's NJ / untiled choice, rp_critic_bwd's dx_cols_ok (first_layer_dx),
rows_grid / bwd_rows_grid of net_pass.h, k_rp_sample's 256 / A rows per workgroup):

| case      | Hp / Hc   | A  | NB  | K  | B             | also                               | paths                                       |
|-----------|-----------|----|-----|----|---------------|------------------------------------|---------------------------------------------|
| default   | 512 / 512 | 12 | 151 | 16 | 4096          | O=48, v +-100, old policy differs  | policy head dW NJ=8, RMS NJ=8, the          |
|           |           |    |     |    |               |                                    | reference's defaults                        |
| widest    | 768 / 768 | 32 | 256 | 4  | 1000          | old policy differs                 | dx-cols fallback (stage_dx over Oc + A), all|
|           |           |    |     |    |               |                                    | heads untiled, RMS NJ=12, 4th softmax slot, |
|           |           |    |     |    |               |                                    | ragged row tiles                            |
| act64     | 64 / 512  | 64 | 65  | 2  | 333           | Oc + A = 77 (not a multiple of 4)  | dx-cols fallback at A=64, k_rp_sample 4     |
|           |           |    |     |    |               |                                    | rows per workgroup, NB one past a wave slot |
| narrow    | 192 / 320 | 1  | 2   | 1  | 37            | policy_min_std 0.05, aux 0.5,      | RMS NJ 3 and 5, 256 rows per workgroup,     |
|           |           |    |     |    |               | targets beyond +-v, old differs    | NB=2, the target clamp                      |
| tiles     | 128 / 128 | 17 | 151 | 64 | 4097          | old policy differs                 | critic and pred head dW NJ=12, 15 rows per  |
|           |           |    |     |    |               |                                    | workgroup with an idle lane, split-operand  |
|           |           |    |     |    |               |                                    | weight-gradient engine with a ragged tail   |
| many_rows | 64 / 64   | 3  | 21  | 4  | 64 num_cus+37 |                                    | backward RMS grid-stride loop (num_cus read |
|           |           |    |     |    |               |                                    | from the device)                            |

Where the profiler sees the path it is asserted: the policy step of a fallback case launches k_gemm_dx with Kd = Oc + A (the
critic's whole input gradient); the others take launch_dx_cols and launch no k_gemm_dx of that width.

Also: act / evaluate_next at A=1, A=64, hidden 768 and above the forward row-grid cap (policy_min_std > 0); the whole update
at the reference's default size against the same 512 single steps, bit for bit; the observation normaliser at the plugin's
sizes past a float32 count of 1e6; and the envelope's refusals for every rlx_reppo_* entry point."""
import re

import numpy as np
import pytest
import torch

import reppo_twin as tw
from reppo_cases import Case, _close, _f32, _hp, _rel, _t, _with_noise, place_kl_bound, value_floor
from rlx_amd.hip import reppo_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _shape_case(name):
    """name -> (Case kwargs, critic input gradient through the stage_dx fallback).  The old policy's samples are injected at
    half the N(0, 1) scale: with up to 4.5M of them (tiles) the N(0, 1) tails push old bases to |9|, where float32's rounding of
    the old action a moves atanh(a) by ulp / (1 - a^2) -- the twin then differs from any float32 computation by up to 2e-5 in
    the gradient and 2x the bar in the KL (measured), which would measure float32's conditioning instead of the kernels.  At
    half scale that share is below 1e-7; the clamp region itself is pinned against the reference by the fixture (case 3)"""
    kw = {
        "default": (dict(seed=41, B=4096, O=48, A=12, Hp=512, Hc=512, NB=151, nr_kl_samples=16, v_min=-100.0, v_max=100.0, old_seed=91),
                    False),
        "widest": (dict(seed=42, B=1000, A=32, Hp=768, Hc=768, NB=256, nr_kl_samples=4, old_seed=92), True),
        "act64": (dict(seed=43, B=333, A=64, Hp=64, Hc=512, NB=65, nr_kl_samples=2), True),
        "narrow": (dict(seed=44, B=37, A=1, Hp=192, Hc=320, NB=2, nr_kl_samples=1, policy_min_std=0.05, auxiliary_loss_coefficient=0.5,
                        targets_beyond=True, old_seed=94), False),
        "tiles": (dict(seed=45, B=4097, A=17, Hp=128, Hc=128, NB=151, nr_kl_samples=64, old_seed=95), False),
        "many_rows": (dict(seed=46, B=64 * _num_cus() + 37, A=3, Hp=64, Hc=64, NB=21, nr_kl_samples=4), False),
    }[name]
    return dict(kw[0], eps_old_scale=0.5), kw[1]


NAMES = ["default", "widest", "act64", "narrow", "tiles", "many_rows"]


def _dx_cols_ok(K, nc):
    """mlp.hip dx_cols_ok: launch_dx_cols takes at most 64 columns with a 16-row tile of 16 (K + 4) + K nc floats in 128 KB"""
    return 1 <= nc <= 64 and K % 4 == 0 and (16 * (K + 4) + K * nc) * 4 <= 128 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_shape_case_reaches_its_paths(name):
    """the case table's claims, from the host selection code's arithmetic (fs_head_bwd, dx_cols_ok, the row grids)"""
    kw, fallback = _shape_case(name)
    c = Case(**kw)
    Oc = len(c.cidx)
    assert _dx_cols_ok(c.Hc, c.A) != fallback

    def head_nj(K, N):     # fs_head_bwd: 0 = the untiled kernel
        TK = K // 8
        TN = 256 // TK if 0 < TK <= 256 else 0
        nj = -(-N // TN) if TN else 99
        if not (K % 8 == 0 and nj <= 12 and 16 * (K + N) * 4 <= 48 * 1024):
            return 0
        return 2 if nj <= 2 else 4 if nj <= 4 else 8 if nj <= 8 else 12
    nj = (head_nj(c.Hp, 2 * c.A), head_nj(c.Hc, c.NB), head_nj(c.Hc, c.Hc + 1))
    want = {"default": lambda: nj[0] == 8 and c.Hp // 64 == 8 and c.h["v_max"] == 100.0 and c.O == 48,
            "widest": lambda: nj == (0, 0, 0) and c.Hc // 64 == 12 and c.NB > 192 and c.B % 16 != 0 and c.B % 128 != 0,
            "act64": lambda: 256 // c.A == 4 and c.NB == 65 and (Oc + c.A) % 4 != 0,
            "narrow": lambda: {c.Hp // 64, c.Hc // 64} == {3, 5} and 256 // c.A == 256 and c.NB == 2 and (np.abs(c.targets) > 10).sum() >= 4,
            "tiles": lambda: nj[1] == 12 and nj[2] == 12 and 256 // c.A == 15 and 256 % c.A != 0 and c.B >= 4096 and c.B % 128 != 0,
            "many_rows": lambda: -(-c.B // 16) > 4 * _num_cus() and c.B % 16 != 0}[name]
    assert want(), (name, nj)


def _gemm_dx_widths(ctx, fn):
    ctx.prof_begin()
    try:
        fn()
    finally:
        ctx.prof_end()
    return {(r["M"], r["N"], r["K"]) for r in ctx.prof_rows() if r["kernel"] == "k_gemm_dx"}


@pytest.mark.parametrize("name", NAMES)
def test_critic_step_matches_the_twin(ctx, dev, name):
    c = place_kl_bound(Case(**_shape_case(name)[0]))
    hp = _hp(c.h)
    Q, qm, qv = _t(c.q, dev), torch.zeros(c.q.size, device=dev), torch.zeros(c.q.size, device=dev)
    met = torch.zeros(5, device=dev)
    rows = np.random.default_rng(3).permutation(c.B).astype(np.int32)
    lr = 3e-4
    if name == "narrow":        # the clamp matters: rows with targets past the support are counted in the loss
        assert ((np.abs(c.targets[rows]) > c.h["v_max"]) & (c.truncs[rows] == 0)).sum() >= 2
    for step in (1, 2):       # two steps: the second one sees non-zero Adam moments
        q0 = Q.cpu().numpy()
        ctx.reppo_critic_step(c.desc, Q, qm, qv, c.batch_dev(dev), step, lr, hp, met, rows=_t(rows, dev, np.int32),
                              cidx=_t(c.cidx, dev, np.int32))
        tb = tuple(x[rows] for x in c.batch_twin())
        pm_, pv_ = (np.zeros(c.q.size), np.zeros(c.q.size)) if step == 1 else (prev_m, prev_v)
        rq, rm, rv, rmet, g = tw.critic_step(q0, pm_, pv_, step, lr, c.LQ, tb, c.h)
        got = met.cpu().numpy()
        for k in range(5):
            assert abs(got[k] - rmet[k]) <= 1e-5 * max(abs(rmet[k]), 1.0), (k, got, rmet)
        assert _rel(Q.cpu().numpy() - q0, _f32(rq) - q0) < 2e-4
        assert _rel(qm.cpu().numpy(), rm) < 1e-5 and _rel(qv.cpu().numpy(), rv) < 5e-5
        prev_m, prev_v = qm.cpu().numpy().astype(np.float64), qv.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", NAMES)
def test_policy_step_matches_the_twin(ctx, dev, name):
    kw, fallback = _shape_case(name)
    c = place_kl_bound(Case(**kw))
    hp = _hp(c.h)
    P, pm, pv = _t(c.p, dev), torch.zeros(c.p.size, device=dev), torch.zeros(c.p.size, device=dev)
    OP, Q = _t(c.old_p, dev), _t(c.q, dev)
    met = torch.zeros(9, device=dev)
    en, eo = _t(c.eps_new, dev), _t(c.eps_old, dev)
    q_before = Q.clone()
    step = lambda: _with_noise(ctx, en, eo, lambda: ctx.reppo_policy_step(c.desc, P, pm, pv, OP, Q, _t(c.states, dev), L.prng_key(1), 1, 3e-4,
                                                                          hp, met, pidx=_t(c.pidx, dev, np.int32),
                                                                          cidx=_t(c.cidx, dev, np.int32)))
    dx = _gemm_dx_widths(ctx, step)
    full = (c.B, len(c.cidx) + c.A, c.Hc)            # the critic's whole input gradient: M = B, Kd = Oc + A, N = Hc
    assert (full in dx) == fallback, (sorted(dx), full)
    # the twin with the old actions rounded to float32 before atanh, as the float32 reference and the kernel compute them
    rp, rm, rv, rmet, g, kl = tw.policy_step(c.p, np.zeros(c.p.size), np.zeros(c.p.size), c.old_p, c.q, 1, 3e-4, c.LP, c.LQ,
                                             c.states[:, c.pidx], c.states[:, c.cidx], c.eps_new, c.eps_old, c.h, f32_old_action=True)
    assert torch.equal(Q, q_before)
    inside = kl < c.h["kl_bound"]
    if c.old_p is c.p:
        assert inside.all()
    else:
        assert 0 < inside.sum() < len(kl)                          # both branches of the where
    got = met.cpu().numpy()
    for k in range(9):
        tol = 1e-5 * max(abs(rmet[k]), 1.0) if k != 4 else 1e-5 * max(abs(rmet[k]), 0.1)
        assert abs(got[k] - rmet[k]) <= tol, (k, got, rmet)
    gp = pm.cpu().numpy() / 0.1 * (min(1.0, hp.max_grad_norm / (rmet[8] + 1e-6)) ** -1)   # m_1 = 0.1 x clipped gradient
    assert _rel(gp, g) < (2e-5 if c.B >= 4096 else 1e-5)
    assert _rel(gp[c.LP["coef"]:], g[c.LP["coef"]:]) < 1e-5
    sel = np.abs(g) > 1e-3 * np.sqrt(np.mean(g * g))
    assert sel.mean() > 0.9
    assert _rel((P.cpu().numpy() - c.p)[sel], (_f32(rp) - c.p)[sel]) < 2e-4 and _rel(pv.cpu().numpy(), rv) < 5e-5


def _act_cases():
    return {"a1": dict(N=300, A=1, Hp=64, Hc=64, NB=21),
            "a64": dict(N=301, A=64, Hp=64, Hc=128, NB=65),
            "h768": dict(N=257, A=6, Hp=768, Hc=768, NB=256, v_min=-100.0, v_max=100.0),
            "rows": dict(N=32 * _num_cus() + 29, A=3, Hp=64, Hc=64, NB=51)}   # above rows_grid's cap: a second grid-stride pass


@pytest.mark.parametrize("name", ["a1", "a64", "h768", "rows"])
def test_act_and_evaluate_next_match_the_twin(ctx, dev, name):
    kw = dict(_act_cases()[name])
    N = kw.pop("N")
    c = Case(7, N, policy_min_std=0.05, **kw)
    hp = _hp(c.h)
    obs = c.states
    rng = np.random.default_rng(8)
    low = -1.0 - rng.random(c.A)
    high = low + 0.5 + 2.0 * rng.random(c.A)
    P, Q = _t(c.p, dev), _t(c.q, dev)
    pidx, cidx = _t(c.pidx, dev, np.int32), _t(c.cidx, dev, np.int32)
    act, proc = torch.empty(N, c.A, device=dev), torch.empty(N, c.A, device=dev)
    eps = _t(c.eps_new, dev)
    key = L.prng_key(5)
    _with_noise(ctx, eps, None, lambda: ctx.reppo_act(c.desc, P, _t(obs, dev), key, act, proc, _t(low, dev), _t(high, dev), hp, pidx=pidx))
    ra, rp = tw.act(c.p, c.LP, obs[:, c.pidx], c.eps_new, c.h, low, high)
    assert _rel(act.cpu().numpy(), ra) < 1e-5 and _rel(proc.cpu().numpy(), rp) < 1e-5
    ctx.reppo_act(c.desc, P, _t(obs, dev), key, act, proc, _t(low, dev), _t(high, dev), hp, True, pidx=pidx)
    assert _rel(act.cpu().numpy(), tw.act(c.p, c.LP, obs[:, c.pidx], None, c.h, low, high, True)[0]) < 1e-5
    nf, nv, sr = torch.empty(N, c.Hc, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    _with_noise(ctx, eps, None, lambda: ctx.reppo_evaluate_next(c.desc, P, Q, _t(obs, dev), _t(c.rewards, dev), key, nf, nv, sr, hp, pidx,
                                                                cidx))
    F, v, s = tw.evaluate_next(c.p, c.LP, c.q, c.LQ, obs[:, c.pidx], obs[:, c.cidx], c.rewards, c.eps_new, c.h)
    assert _rel(nf.cpu().numpy(), F) < 1e-5 and _close(nv.cpu().numpy(), v, value_floor(c.h)) and _rel(sr.cpu().numpy(), s) < 1e-5


def test_whole_update_at_the_default_size_equals_single_steps(ctx, dev):
    """rlx_reppo_update_f32 at the reference's defaults (4096 envs x 128 steps, 4 epochs x 128 minibatches, hidden 512, 151 bins,
    v +-100, 16 KL samples, O = 48) == the same 512 critic + policy steps, bit for bit (threefry noise): every metrics row, the
    final parameters and moments, the key.  The first minibatch's metrics against the twin.  The batch is drawn on the device
    (next_features alone is 1 GB); float64 host copies are taken of the first minibatch's rows only."""
    envs, steps, epochs, mbs = 4096, 128, 4, 128
    batch, mb = envs * steps, envs * steps // mbs
    c = Case(51, 8, O=48, A=12, Hp=512, Hc=512, NB=151, old_seed=93, nr_kl_samples=16, v_min=-100.0, v_max=100.0)
    hp = _hp(c.h)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    rn = lambda *sh: torch.randn(*sh, device=dev, generator=gen)
    states = rn(batch, c.O)
    actions = torch.tanh(rn(batch, c.A))
    rewards, targets = rn(batch) * 2.0, rn(batch) * 60.0          # TD-lambda targets over the +-100 support, some beyond it
    next_features = rn(batch, c.Hc) * 0.5
    u = torch.rand(batch, device=dev, generator=gen)
    terms = (u < 0.2).float()
    truncs = ((u >= 0.2) & (u < 0.35)).float()
    bd = (states, actions, rewards, targets, next_features, terms, truncs)
    perm = torch.stack([torch.randperm(batch, device=dev, generator=gen) for _ in range(epochs)]).to(torch.int32).contiguous()
    pidx, cidx = _t(c.pidx, dev, np.int32), _t(c.cidx, dev, np.int32)
    z = lambda n: torch.zeros(n, device=dev)
    state0 = [_t(c.p, dev), z(c.p.size), z(c.p.size), _t(c.q, dev), z(c.q.size), z(c.q.size)]
    OP = _t(c.old_p, dev)
    a = [x.clone() for x in state0]
    met = z(epochs * mbs * 14).view(epochs * mbs, 14)
    key0 = L.prng_key(42)
    key, cnt = ctx.reppo_update(c.desc, a[0], a[1], a[2], OP, a[3], a[4], a[5], bd, perm, mbs, key0, 0, 3e-4, hp, met, pidx=pidx, cidx=cidx)
    assert cnt == epochs * mbs and torch.isfinite(met).all()
    b = [x.clone() for x in state0]
    k = key0
    ref = z(14)
    flat = perm.view(-1)
    for i in range(epochs * mbs):
        rows = flat[i * mb:(i + 1) * mb]
        ctx.reppo_critic_step(c.desc, b[3], b[4], b[5], bd, i + 1, 3e-4, hp, ref[:5], rows=rows, cidx=cidx)
        k = ctx.reppo_policy_step(c.desc, b[0], b[1], b[2], OP, b[3], states, k, i + 1, 3e-4, hp, ref[5:], rows=rows, pidx=pidx, cidx=cidx)
        assert torch.equal(ref, met[i]), i
    assert np.array_equal(k, key)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the first minibatch against the twin: critic step, then the policy step on the updated critic with injected noise (the same
    # call again from the initial state; only its first minibatch is compared)
    rows = flat[:mb].long()
    host = lambda x: x[rows].cpu().numpy().astype(np.float64)
    s_rows = host(states)
    tb = (s_rows[:, c.cidx], host(actions), host(targets), host(rewards), next_features[rows].cpu().numpy(), host(terms), host(truncs))
    assert (np.abs(tb[2]) > 100.0).any()
    rq, _, _, rmet, _ = tw.critic_step(c.q, np.zeros(c.q.size), np.zeros(c.q.size), 1, 3e-4, c.LQ, tb, c.h)
    got = met[0, :5].cpu().numpy()
    for j in range(5):
        assert abs(got[j] - rmet[j]) <= 1e-5 * max(abs(rmet[j]), 1.0), (j, got, rmet)
    rng = np.random.default_rng(5)
    en = rng.standard_normal((mb, c.A)).astype(np.float32)
    eo = rng.standard_normal((c.h["nr_kl_samples"], mb, c.A)).astype(np.float32)
    a = [x.clone() for x in state0]
    ten, teo = _t(en, dev), _t(eo, dev)
    _with_noise(ctx, ten, teo, lambda: ctx.reppo_update(c.desc, a[0], a[1], a[2], OP, a[3], a[4], a[5], bd, perm[:1].contiguous(), mbs, key0,
                                                        0, 3e-4, hp, met[:mbs], pidx=pidx, cidx=cidx))
    _, _, _, pmet, _, _ = tw.policy_step(c.p, np.zeros(c.p.size), np.zeros(c.p.size), c.old_p, rq, 1, 3e-4, c.LP, c.LQ,
                                         s_rows[:, c.pidx], s_rows[:, c.cidx], en, eo, c.h)
    got = met[0, 5:].cpu().numpy()
    for j in range(9):
        tol = 1e-5 * max(abs(pmet[j]), 1.0) if j != 4 else 1e-5 * max(abs(pmet[j]), 0.1)
        assert abs(got[j] - pmet[j]) <= tol, (j, got, pmet)


def test_observation_normaliser_at_the_plugin_sizes(ctx, dev):
    """N = 4096 rows (the plugin's nr_envs), O = 48, past a float32 count of 1e6: some columns with a mean 1000 times their
    spread (mean 50, std 0.05), where a one-pass variance would cancel"""
    rng = np.random.default_rng(10)
    N, O, n_upd = 4096, 48, 250
    mu = np.where(np.arange(O) % 3 == 0, 50.0, rng.standard_normal(O) * 2.0)
    sd = np.where(np.arange(O) % 3 == 0, 0.05, 0.5 + rng.random(O) * 2.0)
    stiff = np.arange(O) % 3 == 0
    mean, var, cnt = torch.zeros(O, device=dev), torch.ones(O, device=dev), torch.full((1,), 1e-4, device=dev)
    m, v, c = np.zeros(O, np.float32), np.ones(O, np.float32), np.float32(1e-4)
    for i in range(n_upd):
        x = (rng.standard_normal((N, O)) * sd + mu + 0.01 * np.sin(i)).astype(np.float32)
        ctx.reppo_obs_norm_update(_t(x, dev), mean, var, cnt)
        m, v, c = tw.obs_norm_update(m, v, c, x)
    assert c > 1e6 and cnt.item() == c                        # the float32 count, step for step
    gm, gv = mean.cpu().numpy(), var.cpu().numpy()
    assert _rel(gm, m) < 1e-5 and _rel(gv, v) < 1e-5
    assert _rel(gv[stiff], v[stiff]) < 1e-5 and np.all(np.abs(gv[stiff] / 0.05 ** 2 - 1.0) < 0.05)
    out = ctx.reppo_obs_norm_apply(_t(x, dev), mean, var, torch.empty(N, O, device=dev))
    # against the device's own statistics: x - mean cancels 50 to 0.05 in the stiff columns, where the float32 means' last
    # bits (5e-6 apart, 1e-7 relative) would move the output by 1e-4
    gm64, gv64 = gm.astype(np.float64), gv.astype(np.float64)
    assert _rel(out.cpu().numpy(), (x - gm64) / np.sqrt(gv64 + np.float32(1e-8))) < 1e-5


# ------------------------------------------------------------------------------------------------------------- refusals
EINVAL, EUNSUP = -1, -4
SENTINEL = 1234.5


def _refusals():
    """(name, desc overrides, hparam overrides, call overrides, code, message fragment)"""
    D = lambda **kw: kw
    return [
        ("hidden0", D(policy_hidden=0), {}, {}, EUNSUP, "multiples of 64, at most 768"),
        ("hidden96", D(critic_hidden=96), {}, {}, EUNSUP, "multiples of 64, at most 768"),
        ("hidden832", D(policy_hidden=832), {}, {}, EUNSUP, "multiples of 64, at most 768"),
        ("bins1", D(nr_bins=1), {}, {}, EUNSUP, "nr_bins in 2..256"),
        ("bins257", D(nr_bins=257), {}, {}, EUNSUP, "nr_bins in 2..256"),
        ("act0", D(act_dim=0), {}, {}, EINVAL, "positive widths"),
        ("act65", D(act_dim=65), {}, {}, EUNSUP, "act_dim at most 64"),
        ("kl0", {}, dict(nr_kl_samples=0), {}, EINVAL, "nr_kl_samples <= 1024"),
        ("kl1025", {}, dict(nr_kl_samples=1025), {}, EINVAL, "nr_kl_samples <= 1024"),
        ("v_equal", {}, dict(v_min=5.0, v_max=5.0), {}, EINVAL, "v_max > v_min"),
        ("minibatches", {}, {}, dict(nr_minibatches=7), EINVAL, "multiple of nr_minibatches"),
        ("no_pidx", {}, {}, dict(pidx=None), EINVAL, "needs"),
        ("no_cidx", {}, {}, dict(cidx=None), EINVAL, "needs"),
    ]


# which entry points check what: act has no rlx_reppo_hparams limits (it reads policy_min_std only) and no critic columns;
# the critic step reads no policy columns; only the whole update takes a minibatch count
_APPLIES = {"act": lambda n, h, k: not h and "cidx" not in k and "nr_minibatches" not in k,
            "evaluate_next": lambda n, h, k: "nr_minibatches" not in k,
            "critic_step": lambda n, h, k: "nr_minibatches" not in k and "pidx" not in k,
            "policy_step": lambda n, h, k: "nr_minibatches" not in k,
            "update": lambda n, h, k: True}
REFUSALS = [(e, r) for e in _APPLIES for r in _refusals() if _APPLIES[e](r[0], r[2], r[3])]


@pytest.mark.parametrize("entry,r", REFUSALS, ids=["%s-%s" % (e, r[0]) for e, r in REFUSALS])
def test_envelope_refusals(ctx, dev, entry, r):
    """a value just outside each limit: the documented code, rlx_last_error() names the limit, nothing is written (outputs
    prefilled with a sentinel, parameters, moments and the key unchanged), and the context runs a valid call afterwards"""
    name, dover, hover, kover, code, msg = r
    O, A, Hp, Hc, NB, B = 11, 3, 64, 64, 21, 32
    base = dict(policy_obs_dim=9, critic_obs_dim=O, act_dim=A, policy_hidden=Hp, critic_hidden=Hc, nr_bins=NB)
    c = Case(61, B, O=O, A=A, Hp=Hp, Hc=Hc, NB=NB)
    dd = dict(base, **dover)
    if "pidx" in kover or "cidx" in kover:     # the refused width: != O on the side whose indices are missing
        dd["critic_obs_dim"] = O - 1 if "cidx" in kover else O
    desc = reppo_desc(*(dd[k] for k in ("policy_obs_dim", "critic_obs_dim", "act_dim", "policy_hidden", "critic_hidden", "nr_bins")))
    h = dict(c.h, **hover)
    hp = _hp(h)
    fill = lambda *sh: torch.full(sh, SENTINEL, device=dev)
    P, Q, OP = _t(c.p, dev), _t(c.q, dev), _t(c.p, dev)
    pm, pv, qm, qv = fill(c.p.size), fill(c.p.size), fill(c.q.size), fill(c.q.size)
    P0, Q0 = P.clone(), Q.clone()
    pidx = None if kover.get("pidx", 1) is None else _t(np.arange(9), dev, np.int32)
    cidx = None if kover.get("cidx", 1) is None else _t(np.arange(dd["critic_obs_dim"]), dev, np.int32)
    states = _t(c.states, dev)
    bd = c.batch_dev(dev)
    outs = []
    key = L.prng_key(3)

    def call():
        if entry == "act":
            outs.extend([fill(B, A), fill(B, A)])
            return ctx.reppo_act(desc, P, states, key, outs[0], outs[1], _t(-np.ones(A), dev), _t(np.ones(A), dev), hp, pidx=pidx)
        if entry == "evaluate_next":
            outs.extend([fill(B, Hc), fill(B), fill(B)])
            return ctx.reppo_evaluate_next(desc, P, Q, states, bd[2], key, outs[0], outs[1], outs[2], hp, pidx, cidx)
        if entry == "critic_step":
            outs.append(fill(5))
            return ctx.reppo_critic_step(desc, Q, qm, qv, bd, 1, 3e-4, hp, outs[0], cidx=cidx)
        if entry == "policy_step":
            outs.append(fill(9))
            return ctx.reppo_policy_step(desc, P, pm, pv, OP, Q, states, key, 1, 3e-4, hp, outs[0], pidx=pidx, cidx=cidx)
        mbs = kover.get("nr_minibatches", 2)
        outs.append(fill(2 * mbs, 14))
        perm = _t(np.stack([np.arange(B)] * 2), dev, np.int32)
        return ctx.reppo_update(desc, P, pm, pv, OP, Q, qm, qv, bd, perm, mbs, key, 0, 3e-4, hp, outs[0], pidx=pidx, cidx=cidx)
    with pytest.raises(L.RlxError) as e:
        call()
    text = str(e.value)
    rc = int(re.search(r"rc=(-?\d+)", text).group(1))
    assert rc == code and msg in text, text
    assert msg in L.load_library().rlx_last_error().decode()
    torch.cuda.synchronize()
    for t in outs + [pm, pv, qm, qv]:
        assert bool((t == SENTINEL).all()), entry
    assert torch.equal(P, P0) and torch.equal(Q, Q0)
    # the context still serves a valid call
    good = Case(62, B, O=O, A=A, Hp=Hp, Hc=Hc, NB=NB)
    met = torch.zeros(5, device=dev)
    ctx.reppo_critic_step(good.desc, _t(good.q, dev), torch.zeros(good.q.size, device=dev), torch.zeros(good.q.size, device=dev),
                          good.batch_dev(dev), 1, 3e-4, _hp(good.h), met, cidx=_t(good.cidx, dev, np.int32))
    torch.cuda.synchronize()
    assert torch.isfinite(met).all() and met[4].item() > 0
