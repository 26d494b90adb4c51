"""GPU: rlx_tqc_quantile_loss_f32 alone (k_tqc_target, k_tqc_qloss) against numpy float64 on the same float32 inputs.

Bars: y at 1e-6 of the magnitude of its terms |r| + gamma (1 - term) (|z| + alpha |logp'|) -- y is a sum that can cancel, so an
element's own value is no scale for a float32 result (five roundings of at most 2^-24 each stay below 3e-7 of that magnitude) --
and 1e-6 relative L2 over the matrix; the rows non-decreasing; the loss at 1e-5 relative; dq at 1e-5 relative L2.  The float64 sort of
the same float32 values picks the same multiset, and the loss and its gradient are continuous at delta = 0 and |delta| = kappa,
so no margins around the kinks."""
import numpy as np
import pytest
import torch

import tqc_twin as tw
from rlx_amd.hip import RlxError, TqcHparams

pytestmark = pytest.mark.gpu

GAMMA = 0.99
# (E, N, dropped): every slot of the hand-indexed kernels
SIZES = [(1, 1, 0),      # smallest size
         (2, 1, 0),      # smallest ensemble
         (2, 25, 2),     # the default
         (2, 32, 0),     # exactly one atom per lane, no truncation
         (5, 13, 1),     # first atom in the second slot
         (5, 25, 2),     # the paper's size
         (4, 32, 31),    # full wave, K = E
         (8, 16, 3)]     # full wave, larger ensemble


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _hp(E, N, dropped, kappa=1.0):
    return TqcHparams(GAMMA, 0.005, -1.0, -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8, kappa, E, N, dropped)


def _inputs(seed, E, N, B, spread=1.0):
    rng = np.random.default_rng(seed)
    f = lambda x: x.astype(np.float32)
    return dict(q=f(spread * rng.standard_normal((E, B, N))), z=f(spread * rng.standard_normal((E, B, N))), r=f(rng.standard_normal(B)),
                term=f(rng.random(B) < 0.2), lp=f(rng.standard_normal(B) - 1.0), la=np.float32(-0.3))


def _pooled(x):          # [E, B, N] -> [B, T], column e N + n
    E, B, N = x.shape
    return x.transpose(1, 0, 2).reshape(B, E * N).astype(np.float64)


def _run(ctx, dev, d, hp, want_y=True):
    E, B, N = d["q"].shape
    K = E * N - E * hp.nr_dropped_atoms_per_net
    dq, loss = torch.full((E, B, N), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    y = torch.full((B, K), 7.0, device=dev) if want_y else None
    ctx.tqc_quantile_loss(_t(d["q"], dev), _t(d["z"], dev), _t(d["r"], dev), _t(d["term"], dev), _t(d["lp"], dev),
                          _t(np.array([d["la"]]), dev), hp, dq, loss, y)
    torch.cuda.synchronize()
    return dq.cpu().numpy(), float(loss.item()), None if y is None else y.cpu().numpy()


def _reference(d, hp):
    E, B, N = d["q"].shape
    K = E * N - E * hp.nr_dropped_atoms_per_net
    f = lambda x: x.astype(np.float64)
    alpha = np.exp(np.float64(d["la"]))
    y = tw.truncated_target(_pooled(d["z"]), f(d["r"]), f(d["term"]), alpha, f(d["lp"]), GAMMA, K)
    loss, dq = tw.pair_loss(_pooled(d["q"]), y, float(hp.huber_kappa))
    scale = np.abs(f(d["r"]))[:, None] + GAMMA * (1 - f(d["term"]))[:, None] * (
        np.sort(np.abs(_pooled(d["z"])), axis=1)[:, -1:] + alpha * np.abs(f(d["lp"]))[:, None])
    return y, scale, loss.mean(), dq.reshape(B, E, N).transpose(1, 0, 2)


def _check(ctx, dev, d, hp, label):
    dq, loss, y = _run(ctx, dev, d, hp)
    y_e, scale, loss_e, dq_e = _reference(d, hp)
    ey = float(np.max(np.abs(y - y_e) / scale))
    ry = float(np.linalg.norm(y - y_e) / max(np.linalg.norm(y_e), 1e-30))
    rd = float(np.linalg.norm(dq - dq_e) / np.linalg.norm(dq_e))
    rl = abs(loss - loss_e) / abs(loss_e)
    print(f"tqc loss {label}: y {ey:.1e} of its terms, {ry:.1e} L2; loss {rl:.1e}; dq {rd:.1e}")
    assert np.all(np.diff(y, axis=1) >= 0), label
    assert ey <= 1e-6 and ry <= 1e-6, (label, ey, ry)
    assert rl <= 1e-5, (label, loss, loss_e)
    assert rd <= 1e-5, (label, rd)
    return dq, loss, y


@pytest.mark.parametrize("B", [1, 13, 1000])                     # 13: idle waves in the last workgroup
@pytest.mark.parametrize("E,N,dropped", SIZES)
def test_quantile_loss_matches_float64(ctx, dev, E, N, dropped, B):
    _check(ctx, dev, _inputs(1000 * E + 10 * N + B, E, N, B), _hp(E, N, dropped), f"E={E} N={N} drop={dropped} B={B}")


def test_duplicate_atoms(ctx, dev):
    """critic 1's next atoms copied from critic 0: every value occurs twice; the sort moves values, so ties need no rule"""
    d = _inputs(5, 2, 25, 13)
    d["z"][1] = d["z"][0]
    _, _, y = _check(ctx, dev, d, _hp(2, 25, 2), "duplicates")
    live = d["term"] == 0
    assert np.all(y[live][:, 0:46:2] == y[live][:, 1:46:2])


def test_sorted_and_reverse_sorted_rows(ctx, dev):
    d = _inputs(6, 5, 25, 2)
    z = np.sort(_pooled(d["z"]).astype(np.float32), axis=1)
    z[1] = z[1, ::-1]
    d["z"] = np.ascontiguousarray(z.reshape(2, 5, 25).transpose(1, 0, 2))
    d["term"][:] = 0
    _check(ctx, dev, d, _hp(5, 25, 2), "sorted / reversed")


def test_all_terminated_gives_the_reward(ctx, dev):
    d = _inputs(7, 2, 25, 13)
    d["term"][:] = 1
    _, _, y = _check(ctx, dev, d, _hp(2, 25, 2), "terminated")
    assert np.all(y == d["r"][:, None])


@pytest.mark.parametrize("kappa", [0.25, 4.0])
def test_both_huber_branches(ctx, dev, kappa):
    d = _inputs(8, 5, 25, 13, spread=2.0)
    hp = _hp(5, 25, 2, kappa)
    y_e, _, _, _ = _reference(d, hp)
    delta = np.abs(y_e[:, None, :] - _pooled(d["q"])[:, :, None])
    assert 0.05 < (delta > kappa).mean() < 0.95                  # |delta| spread over both branches
    _check(ctx, dev, d, hp, f"kappa={kappa}")


def test_two_identical_calls_give_identical_bits(ctx, dev):
    d, hp = _inputs(9, 5, 25, 1000), _hp(5, 25, 2)
    a, b = _run(ctx, dev, d, hp), _run(ctx, dev, d, hp)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    c = _run(ctx, dev, d, hp, want_y=False)                      # y_out = NULL: the same loss and gradient
    assert np.array_equal(a[0], c[0]) and a[1] == c[1]


@pytest.mark.parametrize("E,N,dropped,kappa,null,code,word", [
    (3, 43, 0, 1.0, None, -4, "total atoms"),                    # T = 129
    (2, 25, 25, 1.0, None, -1, "nr_dropped_atoms_per_net"),      # dropped = N
    (2, 25, 2, 0.0, None, -1, "huber_kappa"),
    (0, 25, 2, 1.0, None, -1, "ensemble_size"),
    (2, 25, 2, 1.0, "dq_out", -1, "dq_out"),
    (2, 25, 2, 1.0, "loss_out", -1, "loss_out")])
def test_refusals_name_the_argument(ctx, dev, E, N, dropped, kappa, null, code, word):
    B = 4
    x = torch.zeros(max(E, 1), B, N, device=dev)
    v = torch.zeros(B, device=dev)
    dq = None if null == "dq_out" else torch.zeros_like(x)
    loss = None if null == "loss_out" else torch.zeros(1, device=dev)
    with pytest.raises(RlxError) as e:
        ctx.tqc_quantile_loss(x, x, v, v, v, torch.zeros(1, device=dev), _hp(E, N, dropped, kappa), dq, loss, None)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
