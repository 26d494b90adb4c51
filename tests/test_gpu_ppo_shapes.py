"""GPU: the PPO minibatch pass (rlx_ppo_minibatch_fwd_bwd_f32) and the whole update (rlx_ppo_update_f32) against the float64 oracle
(oracle/ppo.py) over the shapes the library's checks accept from 4096 rows on -- the split-operand engine with its specialised
kernels (k_l12fwd, k_l1fwd_mfma, k_dx_l1bwd, k_tail_bx, k_tail32_bx, k_gemm_dw_bx and the twin launches), held to the oracle at one
shape by test_gpu_bench_shapes.py.  The cases, what each reaches and the bars: tests/ppo_cases.py; which kernels a case must run:
the selection mirror in tests/net_paths.py (ppo_pass), asserted here from the profiler rows, so a case that drops to another path
fails instead of passing on the wrong kernel.  tests/test_ppo_cases.py holds the cases' inputs to half of each bar in float32 on the
CPU."""
import numpy as np
import pytest
import torch

import net_paths as npth
import ppo_cases as pc
from oracle import prng
from rlx_amd.hip import PpoHparams, mlp_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _descs(O, hidden, A, act, ln):
    return mlp_desc(O, hidden, A, act, ln, True), mlp_desc(O, hidden, 1, act, ln, False)


def _ran(rows):
    return {(r["kernel"], r["engine"], r["M"], r["N"], r["K"]): r["launches"] for r in rows}


def _minibatch(ctx, dev, c, options, hp, profile=True):
    pd, cd = _descs(c.O, c.hidden, c.A, c.act, c.ln)
    pg, cg, met = torch.zeros(c.ps.n_params, device=dev), torch.zeros(c.cs.n_params, device=dev), torch.zeros(8, device=dev)
    dev_in = [_t(x, dev) for x in (c.states, c.actions, c.logp, c.returns, c.adv, c.idx)]
    rows, open_ = None, False
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        if profile:
            ctx.prof_begin()
            open_ = True
        ctx.ppo_minibatch_fwd_bwd(pd, _t(c.pp, dev), pg, cd, _t(c.cp, dev), cg, met, *dev_in, hp)
        if profile:
            open_ = False
            ctx.prof_end()
            rows = ctx.prof_rows()
    finally:
        if open_:                  # a refused or failed call: the shared context does not keep the profiler open
            ctx.prof_end()
        if "ppo_twin" in options:
            ctx.set_option("ppo_twin", -1)
    torch.cuda.synchronize()
    return met.cpu().numpy(), pg.cpu().numpy(), cg.cpu().numpy(), rows


@pytest.mark.parametrize("name,label", pc.RUNS)
def test_minibatch_pass_vs_float64_oracle(ctx, dev, name, label):
    c = pc.case(name)
    options, mirror_opts = next((o, m) for l, o, m in c.settings() if l == label)
    expect = c.expect(mirror_opts)
    hp = PpoHparams(pc.CLIP, pc.ENT, pc.CC, 0.5, 0.9, 0.999, 1e-8)
    met, gp, gc, rows = _minibatch(ctx, dev, c, options, hp)
    ran = _ran(rows)
    metrics, report = pc.compare(c, met, gp, gc)
    print(f"ppo shape {name} [{label}] twin pass: {expect['twin']}; policy {expect['policy']}; critic {expect['critic']}")
    print(f"ppo shape {name} [{label}] rows:", sorted(ran.items()))
    print(f"ppo shape {name} [{label}] metrics (got, float64, allowed):", {k: tuple(float(f"{x:.6g}") for x in v) for k, v in metrics.items()})
    print(f"ppo shape {name} [{label}] ||dg||/||g|| vs float64:", {k: float(f"{v:.2e}") for k, v in report.items()})
    # the kernels the selection mirror predicts, on the engines it predicts, with its launch counts -- and no others
    bad = {k: (ran.get(k), expect["rows"].get(k)) for k in set(ran) | set(expect["rows"]) if ran.get(k) != expect["rows"].get(k)}
    assert not bad, bad
    for k, (got, exp, allowed) in metrics.items():
        assert abs(got - exp) <= allowed, (k, got, exp, allowed)
    for k, v in report.items():
        assert v < pc.GRAD_BAR, (k, v)


@pytest.mark.parametrize("name", sorted(pc.REFUSED))
def test_refused_shapes_answer_with_their_message_and_leave_the_context_usable(ctx, dev, name):
    O, hidden, A, act, ln, mb = pc.REFUSED[name]
    code, msg = npth.ppo_refusal(O, hidden, A, act, ln, mb)
    pd, cd = _descs(O, hidden, A, act, ln)
    B = 2 * mb
    z = lambda *s: torch.zeros(*s, device=dev)
    hp = PpoHparams(pc.CLIP, pc.ENT, pc.CC, 0.5, 0.9, 0.999, 1e-8)
    idx = torch.arange(mb, dtype=torch.int32, device=dev)
    n = npth.mlp_blocks(O, hidden, max(A, 1), ln, True)[1] + 1024
    with pytest.raises(L.RlxError) as e:
        ctx.ppo_minibatch_fwd_bwd(pd, z(n), z(n), cd, z(n), z(n), z(8), z(B, O), z(B, A), z(B), z(B), z(B), idx, hp)
    assert msg in str(e.value) and f"rc={code}" in str(e.value), str(e.value)
    # the context serves the next call, and serves it right
    c = pc.case("one_layer")
    met, gp, gc, _ = _minibatch(ctx, dev, c, {}, hp, profile=False)
    metrics, report = pc.compare(c, met, gp, gc)
    assert all(abs(got - exp) <= allowed for got, exp, allowed in metrics.values()) and max(report.values()) < pc.GRAD_BAR


@pytest.mark.parametrize("name,entry", [(n, "update") for n in pc.UPDATE_NAMES] + [(n, "dist") for n in pc.DIST_NAMES])
def test_whole_update_past_the_first_adam_step_vs_float64_oracle(ctx, dev, name, entry):
    """T = 2, N = mb, two epochs: four updates of mb rows with global-norm clipping active, against oppo.update in float64 from the
    same key (the permutation is bit-exact: both sides draw the same minibatches).  A weight image that Adam left stale, a kept
    gather or a grouped schedule shows here; the wide cases gather their rows at a padded stride (k_gather_rec, the group buffers'
    offsets).  entry "dist": rlx_ppo_update_dist_f32 as the one rank that holds every row -- the same updates.  Bars: the first update
    as the minibatch pass, later updates rtol 2e-3 / atol 2e-5 (test_gpu_twin_update.py), final parameters as test_gpu_errors.py
    (0.999 of the entries within 2e-5 + 1e-3 |e|, all within 2 lr n_upd; tests/test_ppo_cases.py: the float32 numpy update leaves
    out no entry and stays ten times inside the rest)."""
    c = pc.case(name)
    out, key_e, p_e, c_e, n_e = c.update64
    mb, E = c.mb, pc.UPD_EPOCHS
    n_upd = 2 * E
    pd, cd = _descs(c.O, c.hidden, c.A, c.act, c.ln)
    hp = PpoHparams(pc.CLIP, pc.ENT, pc.CC, c.max_grad_norm, 0.9, 0.999, 1e-8)
    P, C = _t(c.pp, dev), _t(c.cp, dev)
    pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
    met = torch.zeros(n_upd, 10, device=dev)
    sh = lambda a, *s: _t(a.reshape(2, mb, *s), dev)
    rollout = (sh(c.states, c.O), sh(c.actions, c.A), sh(c.logp), sh(c.returns), sh(c.adv))
    lr = np.full(n_upd, pc.LR, np.float32)
    ctx.prof_begin()
    try:
        if entry == "dist":
            key, cnt = ctx.ppo_update_dist(pd, P, pm, pv, cd, C, cm, cv, *rollout, mb, 0, E, mb, prng.prng_key(5), 0, lr, hp, met)
        else:
            key, cnt = ctx.ppo_update(pd, P, pm, pv, cd, C, cm, cv, *rollout, E, mb, prng.prng_key(5), 0, lr, hp, met)
        torch.cuda.synchronize()
    finally:
        ctx.prof_end()
    ran = _ran(ctx.prof_rows())
    assert np.array_equal(key, key_e) and cnt == n_e == n_upd
    m = met.cpu().numpy().astype(np.float64)
    cols = {"loss/policy_gradient_loss": 0, "loss/critic_loss": 1, "loss/entropy_loss": 2, "policy_ratio/approx_kl": 3,
            "policy_ratio/clip_fraction": 4, "gradients/policy_grad_norm": 8, "gradients/critic_grad_norm": 9}
    exp = np.array([[float(o[k]) for k in cols] for o in out])
    got = m[:, list(cols.values())]
    print(f"ppo {entry} {name}: metrics |got - float64| / max(|float64|, 1e-3), per update:",
          [[float(f"{x:.1e}") for x in row] for row in np.abs(got - exp) / np.maximum(np.abs(exp), 1e-3)])
    # the pass's own kernels ran in every update -- once per network in the two-chain schedule (the default below 6144 rows), once for
    # both from there to 16384 rows -- and on the exact engine only what the mirror puts there (a wide first layer's forward)
    first = npth.ppo_pass(*c.shape, {"ppo_twin": 1 if npth.twin_default(*c.shape) else 0})
    assert first["twin"] == (name == "mid")
    first = first["rows"]
    bad = {k: (ran.get(k), n * n_upd) for k, n in first.items() if ran.get(k) != n * n_upd}
    assert not bad, (bad, ran)
    assert not any(k[1] == 0 and k not in first for k in ran), ran
    assert all(k[0] == "k_gemm_fwd" and c.O > 32 for k in first if k[1] == 0)
    assert exp[0, 5] > c.max_grad_norm and exp[0, 6] > c.max_grad_norm          # clipping acts
    for i, (k, rtol, atol) in enumerate(pc.METRICS):
        np.testing.assert_allclose(got[0, i], exp[0, i], rtol=rtol, atol=atol, err_msg=k)
    np.testing.assert_allclose(got[0, 4], exp[0, 4], rtol=0, atol=1.5 / mb)
    np.testing.assert_allclose(got[0, 0] - pc.ENT * got[0, 2] + pc.CC * got[0, 1], float(out[0]["loss"]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got[0, 5:7], exp[0, 5:7], rtol=1e-5)
    np.testing.assert_allclose(got[:, [0, 1, 2, 3, 5, 6]], exp[:, [0, 1, 2, 3, 5, 6]], rtol=2e-3, atol=2e-5)
    for which, g, e, start in (("policy", P, p_e, c.pp), ("critic", C, c_e, c.cp)):
        d = np.abs(g.cpu().numpy().astype(np.float64) - e)
        share = (d <= 2e-5 + 1e-3 * np.abs(e)).mean()
        print(f"ppo {entry} {name}: {which} parameters after {n_upd} updates: max |dp| {d.max():.2e}, within 2e-5 + 1e-3 |e|: {share:.6f}")
        assert share > 0.999, (which, d.max(), share)
        assert d.max() <= 2 * pc.LR * n_upd, (which, d.max())
        assert np.abs(e - start).max() > 1e-4, which
