"""GPU: rlx_redq_losses_f32 -- REDQ's critic target / loss / gradient and the policy's min-over-the-ensemble seed on given values --
against the float64 twin (tests/redq_twin.py).  The library's Q matrices are [E, B], the twin's [B, E]."""
import numpy as np
import pytest
import torch

import redq_twin as tw
from rlx_amd.hip import RedqHparams, RlxError

pytestmark = pytest.mark.gpu

GAMMA = 0.99


def _hp(E, M, G=1):
    return RedqHparams(GAMMA, 0.005, -1.0, -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, M, G)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _inputs(B, E, M, seed):
    rng = np.random.default_rng(seed)
    f = lambda x: x.astype(np.float32)
    term = f(rng.random(B) < 0.3)
    term[0] = 1.0                                                      # at least one terminated row: y = r exactly
    return dict(q=f(rng.standard_normal((E, B))), qn=f(rng.standard_normal((M, B))), r=f(rng.standard_normal(B)), term=term,
                nlogp=f(rng.standard_normal(B)), la=np.array([-0.3], np.float32), qa=f(rng.standard_normal((E, B))))


@pytest.mark.parametrize("E,M", [(1, 1), (2, 2), (3, 1), (10, 2), (16, 16)])
@pytest.mark.parametrize("B", [1, 67, 257])
def test_losses_match_twin(ctx, dev, B, E, M):
    x = _inputs(B, E, M, 100 * B + E)
    d = {k: _t(v, dev) for k, v in x.items()}
    y, dq, loss = torch.full((B,), 7.0, device=dev), torch.full((E, B), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    seed, minq = torch.full((E, B), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
    ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), dq, y, loss, d["qa"], seed, minq)
    torch.cuda.synchronize()
    f8 = lambda v: v.astype(np.float64)
    y_e, loss_e, dq_e = tw.critic_loss(f8(x["q"]).T, f8(x["qn"]).T, f8(x["r"]), f8(x["term"]), np.exp(f8(x["la"])[0]), f8(x["nlogp"]), GAMMA)
    rel = lambda got, exp: np.linalg.norm(got.astype(np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)
    figures = (rel(y.cpu().numpy(), y_e), rel(dq.cpu().numpy(), dq_e.T), abs(loss.item() - loss_e.mean()) / loss_e.mean())
    print(f"redq losses B={B} E={E} M={M}: y {figures[0]:.1e} dq {figures[1]:.1e} loss {figures[2]:.1e}")
    assert max(figures) < 1e-6, figures
    done = x["term"] == 1.0
    assert done.any() and np.array_equal(y.cpu().numpy()[done], x["r"][done])          # terminated rows: y = r exactly
    mn_e, seed_e = tw.policy_seed(f8(x["qa"]).T)
    assert np.array_equal(minq.cpu().numpy(), mn_e.astype(np.float32))                 # a min of float32 values is exact
    got = seed.cpu().numpy()
    assert np.array_equal(got != 0, seed_e.T != 0)
    np.testing.assert_allclose(got, seed_e.T, rtol=2e-7, atol=0)
    assert got.sum() == pytest.approx(-1.0, rel=1e-5)


def test_outputs_other_than_the_gradient_may_be_null(ctx, dev):
    B, E, M = 67, 3, 2
    d = {k: _t(v, dev) for k, v in _inputs(B, E, M, 5).items()}
    full = [torch.zeros(B, device=dev), torch.zeros(E, B, device=dev), torch.zeros(1, device=dev)]
    ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), full[1], full[0], full[2])
    dq = torch.zeros(E, B, device=dev)
    ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), dq)
    assert torch.equal(dq, full[1]) and full[2].item() > 0
    seed = torch.zeros(E, B, device=dev)
    ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), dq, qa=d["qa"], seed_out=seed)
    assert seed.sum().item() == pytest.approx(-1.0, rel=1e-5)
    with pytest.raises(RlxError, match="seed_out"):
        ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), dq, qa=d["qa"])
    with pytest.raises(RlxError, match="dq_out"):
        ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), None)
    for hp, word in ((_hp(2, 3), "in_target_minimization_size"), (_hp(17, 1), "ensemble_size")):
        with pytest.raises(RlxError, match=word):
            ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], hp, dq)


@pytest.mark.parametrize("B", [1, 67, 257])
def test_hand_placed_ties_split_the_seed_evenly(ctx, dev, B):
    """E = 4: rows 0 mod 3 have one minimum, rows 1 mod 3 two equal minima (critics 1 and 3), rows 2 mod 3 three (critics 0, 1, 2):
    seeds are exactly -1/B, -1/(2B), -1/(3B) on the tied critics and 0 elsewhere; terminated rows give y = r exactly"""
    E, M = 4, 2
    x = _inputs(B, E, M, 9)
    x["term"][:] = 1.0
    qa = np.abs(x["qa"]) + 1.0                                         # every value above 1; the minima are placed below
    rows = np.arange(B)
    tied = {0: [2], 1: [1, 3], 2: [0, 1, 2]}
    for k, crit in tied.items():
        for e in crit:
            qa[e, rows % 3 == k] = np.float32(-0.25 * (k + 1))
    d = {k: _t(v, dev) for k, v in x.items()}
    y, dq, seed, minq = torch.zeros(B, device=dev), torch.zeros(E, B, device=dev), torch.zeros(E, B, device=dev), torch.zeros(B, device=dev)
    ctx.redq_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, M), dq, y, None, _t(qa, dev), seed, minq)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), x["r"])
    exp = np.zeros((E, B), np.float32)
    for k, crit in tied.items():
        for e in crit:
            exp[e, rows % 3 == k] = np.float32(-1.0) / (np.float32(B) * np.float32(len(crit)))
    assert np.array_equal(seed.cpu().numpy(), exp)
    assert np.array_equal(minq.cpu().numpy(), (-0.25 * (rows % 3 + 1)).astype(np.float32))
