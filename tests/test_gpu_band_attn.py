"""GPU: rlx_band_attn_f32 (attn.hip) against a float64 reference written from the issue's formulas: torch on the CPU, a dense T x T
boolean mask from the three conditions (0 <= i - j < C, seg[i] == seg[j], valid[i] and valid[j]), softmax, autograd.

Everything is compared on rows with valid == 1; dqkv at invalid rows must be exactly 0.  A tensor's bar is 8 times the largest
deviation of the same reference evaluated in float32 on the CPU from its float64 value on that case (the project's margin where only
the summation order differs).

masks() places the breaks and the padding; the tests assert on seg / valid what each case must contain.  Two of the conditions
cannot hold everywhere and are asserted where they can: a break on a tile boundary needs T > 16, "one sequence with a prefix and one
with none" needs S > 1, and a band cut by anything needs C > 1."""
import functools

import numpy as np
import pytest
import torch

from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

#        S, T, nhead, head_dim, C
CASES = [(3, 37, 4, 32, 16), (1, 16, 4, 32, 16), (2, 16, 1, 64, 3), (2, 5, 8, 16, 1), (2, 50, 2, 32, 17), (1, 70, 4, 32, 40),
         (4, 143, 4, 32, 16)]


def masks(S, T, C):
    """seg int32 [S, T], valid uint8 [S, T]: sequence s breaks at token 9 + s (inside a tile), even sequences at 16 (a tile
    boundary) and at 37; sequence 0 starts with min(C - 1, 3) invalid tokens, sequence 2 with min(C - 1, 5), the others with none"""
    seg, valid = np.zeros((S, T), np.int32), np.ones((S, T), np.uint8)
    for s in range(S):
        for b in [min(T - 1, 9 + s)] + ([16, 37] if s % 2 == 0 else []):
            if 0 < b < T:
                seg[s, b:] += 1
        valid[s, :min(C - 1, {0: 3, 2: 5}.get(s, 0), T - 1)] = 0
    return seg, valid


def keep_mask(seg, valid, C):
    """bool [S, T, T]: query i may attend key j"""
    S, T = seg.shape
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    band = (i - j >= 0) & (i - j < C)
    v = valid.astype(bool)
    return band[None] & (seg[:, :, None] == seg[:, None, :]) & v[:, :, None] & v[:, None, :], band


def ref_attn(qkv, keep, nhead, dtype, d_out=None):
    """qkv [S T, 3 D] -> out [S T, D] (and dqkv under the cotangent d_out) in dtype on the CPU"""
    S, T = keep.shape[:2]
    D = qkv.shape[1] // 3
    hd = D // nhead
    x = qkv.to(dtype).reshape(S, T, 3, nhead, hd).clone().requires_grad_()
    logits = torch.einsum("sihd,sjhd->shij", x[:, :, 0] * hd ** -0.5, x[:, :, 1])
    logits = torch.where(keep[:, None], logits, torch.finfo(dtype).min)
    out = torch.einsum("shij,sjhd->sihd", torch.softmax(logits, -1), x[:, :, 2]).reshape(S * T, D)
    if d_out is None:
        return out.detach(), None
    out.backward(d_out.to(dtype))
    return out.detach(), x.grad.reshape(S * T, 3 * D)


@functools.lru_cache(maxsize=None)
def case(S, T, nhead, hd, C):
    """inputs and the float64 reference with its float32 deviations, built once"""
    g = torch.Generator().manual_seed(S * 1000 + T)
    seg, valid = masks(S, T, C)
    keep, _ = keep_mask(seg, valid, C)
    keep = torch.from_numpy(keep)
    rows = torch.from_numpy(valid.reshape(-1).astype(bool))
    qkv = torch.randn(S * T, 3 * nhead * hd, generator=g)
    d_out = torch.randn(S * T, nhead * hd, generator=g) * rows[:, None]
    o64, g64 = ref_attn(qkv, keep, nhead, torch.float64, d_out)
    o32, g32 = ref_attn(qkv, keep, nhead, torch.float32, d_out)
    bars = [8 * float((a32.double() - a64)[rows].abs().max()) for a32, a64 in ((o32, o64), (g32, g64))]
    return seg, valid, rows, qkv, d_out, o64, g64, bars


def run(ctx, dev, c, bwd=True):
    S, T, nhead, hd, C = c
    seg, valid, rows, qkv, d_out = case(*c)[:5]
    out = torch.full((S * T, nhead * hd), float("nan"), device=dev)
    lse = torch.empty(S * T, nhead, device=dev)
    dqkv = torch.full((S * T, 3 * nhead * hd), float("nan"), device=dev)
    ctx.band_attn(qkv.to(dev), torch.from_numpy(seg).to(dev), torch.from_numpy(valid).to(dev), nhead, C, out, lse,
                  d_out.to(dev) if bwd else None, dqkv if bwd else None)
    return out.cpu(), dqkv.cpu()


@pytest.mark.parametrize("c", CASES, ids=str)
def test_forward_and_backward_match_float64(ctx, dev, c):
    S, T, nhead, hd, C = c
    seg, valid, rows, _, _, o64, g64, bars = case(*c)
    keep, band = keep_mask(seg, valid, C)
    v = valid.astype(bool)
    if T > 1:       # what the case must contain (module docstring)
        brk = np.argwhere(seg[:, 1:] != seg[:, :-1])[:, 1] + 1
        assert (brk % 16 != 0).any() and (T <= 16 or (brk % 16 == 0).any())
        prefix = (~v).cumprod(1).sum(1)
        assert C == 1 or ((prefix > 0) & (prefix < C)).any()
        assert S == 1 or (prefix == 0).any()
        cut_seg = band[None] & v[:, :, None] & v[:, None, :] & (seg[:, :, None] != seg[:, None, :])
        cut_pad = band[None] & v[:, :, None] & ~v[:, None, :]
        assert C == 1 or (cut_seg.any() and cut_pad.any())
    out, dqkv = run(ctx, dev, c)
    for name, got, exp, bar in (("out", out, o64, bars[0]), ("dqkv", dqkv, g64, bars[1])):
        err = float((got.double() - exp)[rows].abs().max())
        print(f"{c} {name}: max error {err:.3e}, bar {bar:.3e}, fraction {err / max(bar, 1e-300):.3f}")   # (C = 1: the bar is 0)
        assert err <= bar, (name, err, bar)
    assert torch.all(out[~rows] == 0) and torch.all(dqkv[~rows] == 0)


def test_two_runs_give_identical_bits(ctx, dev):
    a, b = run(ctx, dev, CASES[0]), run(ctx, dev, CASES[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("nhead, hd, C", [(4, 24, 16), (4, 32, 0), (4, 32, 65), (32, 32, 16)], ids=["head_dim", "window0", "window65", "nhead"])
def test_refusals(ctx, dev, nhead, hd, C):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    with pytest.raises(L.RlxError, match=r"rc=-4"):       # RLX_EUNSUP
        ctx.band_attn(z(16, 3 * nhead * hd), z(1, 16, dt=torch.int32), z(1, 16, dt=torch.uint8), nhead, C, z(16, nhead * hd), z(16, nhead))
