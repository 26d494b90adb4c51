"""GPU: the split-K forward GEMM for few rows and a long K (gemm_sk.hip) -- rlx_dbg_gemm_f32 mode 6 against float64 numpy with
asymmetric operands (tests/test_gpu_gemm.py's), at every forced slice count, and through rlx_cnn_net_f32 / rlx_hyper_net_f32 under
the option gemm_small_m = 1 against the references of tests/test_gpu_cnn_net.py and tests/test_gpu_hyper_net.py.  A tensor's bar is
the project's: 8 x max(the same product's float32 numpy deviation from float64 numpy, 2^-24 max |tensor|).

Shapes (M, N, K): (1, 4, 4) one row, one partial strip, a slice shorter than a group of steps, S = 1; (33, 68, 100) a ragged second
row tile, a ragged second column strip, a ragged K tail; (8 | 32, 512, 3136) pqn's and dqn's hidden Dense; (256, 512, 2048) the
SimbaV2 block; (130, 132, 1100) a slice longer than one 512-column LDS stage when S is forced to 1 (the rule gives it S = 8)."""
import functools

import numpy as np
import pytest
import torch

from rlx_amd.hip import lib as L
import test_gpu_cnn_net as cn
import test_gpu_hyper_net as hn

pytestmark = pytest.mark.gpu
SHAPES = [(1, 4, 4), (33, 68, 100), (8, 512, 3136), (32, 512, 3136), (256, 512, 2048), (130, 132, 1100)]
ACT_NONE = 3


@functools.lru_cache(maxsize=None)
def product(M, N, K):
    """-> A, W, b (float32) and A W + b in float64 and in float32 numpy"""
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) * 0.1).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    return A, W, b, A.astype(np.float64) @ W.astype(np.float64) + b, A @ W + b


def run(ctx, dev, shape, act):
    A, W, b, _, _ = product(*shape)
    C = torch.full(shape[:2], float("nan"), device=dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    ctx.dbg_gemm(6, t(A), t(W), C, t(b), *shape, act)
    return C.cpu().numpy()


def check(shape, act, got):
    _, _, _, z64, z32 = product(*shape)
    f = (lambda z: np.maximum(z, 0)) if act == L.ACT_RELU else (lambda z: z)
    bar = 8 * max(np.abs(f(z32) - f(z64)).max(), 2.0 ** -24 * np.abs(f(z64)).max())
    err = np.abs(got - f(z64)).max()
    print(f"{shape} act {act}: max error {err:.3e}, bar {bar:.3e}, fraction {err / bar:.3f}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("act", [ACT_NONE, L.ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mode_6_matches_float64(ctx, dev, shape, act):
    check(shape, act, run(ctx, dev, shape, act))


@pytest.mark.parametrize("S", [1, 2, 0, 64])      # 0: the rule's own count
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[5]], ids=str)
def test_every_slice_count_holds_the_bar_and_repeats_its_bits(ctx, dev, shape, S):
    try:
        ctx.set_option("gemm_sk_slices", S)
        a, b = run(ctx, dev, shape, ACT_NONE), run(ctx, dev, shape, ACT_NONE)
    finally:
        ctx.set_option("gemm_sk_slices", 0)
    check(shape, ACT_NONE, a)
    assert np.array_equal(a, b)


def passes(ctx, dev, c):
    """one call of the public pass of case c -> [(tensor name, got, float64, float32)]"""
    if len(c) == 8:
        _, r64, r32 = cn.case(c)
        out, grads = cn.run(ctx, dev, c)
        g, g64, g32 = (cn.split(t, *c[1:]) for t in (grads, r64["grads"], r32["grads"]))
        return [("out", out, r64["out"], r32["out"])] + [(n, g[n], g64[n], g32[n]) for n in g]
    (desc, params, x, d_out), r64, r32 = hn.case(c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, grads, dx = nan(c[0], c[2]), nan(params.numel()), nan(c[0], c[1])
    ctx.hyper_net(desc, params.to(dev), x.to(dev), out, d_out.to(dev), grads, dx)
    g, g64, g32 = (hn.split(t, *c[1:]) for t in (grads.cpu(), r64["grads"], r32["grads"]))
    return [("out", out.cpu(), r64["out"], r32["out"]), ("dx", dx.cpu(), r64["dx"], r32["dx"])] + [(n, g[n], g64[n], g32[n]) for n in g]


@pytest.mark.parametrize("c", [cn.CASES[1], cn.CASES[2], hn.CASES[2]], ids=str)
def test_the_public_passes_take_the_route_and_hold_their_bars(ctx, dev, c):
    n0 = ctx.get_counter("gemm_sk_launches")
    passes(ctx, dev, c)
    assert ctx.get_counter("gemm_sk_launches") == n0      # option 0: k_gemm_fwd as before
    try:
        ctx.set_option("gemm_small_m", 1)
        got = passes(ctx, dev, c)
    finally:
        ctx.set_option("gemm_small_m", 0)
    assert ctx.get_counter("gemm_sk_launches") > n0
    worst = max(hn.check(c, *t) for t in got)
    print(f"{c}: worst fraction of a bar {worst:.3f}")


def test_refusals(ctx, dev):
    A = torch.zeros(2000, 8, device=dev)
    C = torch.full((2000, 8), float("nan"), device=dev)
    with pytest.raises(L.RlxError, match=r"rc=-4.*M must be"):      # RLX_EUNSUP names the field
        ctx.dbg_gemm(6, A, torch.zeros(8, 8, device=dev), C, torch.zeros(8, device=dev), 2000, 8, 8, ACT_NONE)
    assert bool(torch.isnan(C).all())
    with pytest.raises(L.RlxError, match="rc=-1"):
        ctx.set_option("gemm_small_m", 2)
