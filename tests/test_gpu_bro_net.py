"""GPU: rlx_bro_net_f32 (bro_net.h on bro.hip) -- out, dx and every gradient tensor of the flat layout, per tensor -- against the
formulas of include/rlx_hip.h's section written as a plain torch function on the CPU in float64 (autograd for the backward).  A
tensor's bar is tests/test_gpu_hyper_net.py's: 8 x max(the same function's float32 deviation from float64, 2^-24 max |tensor|).

Layered route with the backward: (1, 17, 64, 1, 0) one row, one chunk, ragged in_dim, no output layer; (33, 23, 512, 2, 100) a ragged
row tile, NQ = 2, the reference critic's shape; (128, 40, 1024, 1, 1) NQ = 4, out_dim below one strip; (4096, 23, 256, 2, 100) the
split-operand engine.  Fused route (fwd_path = 2), forward only: M in {1, 33, 128, 257} on the first three shapes' widths.

The ReLU's backward has a kink at 0: an element whose pre-ReLU value is within rounding of 0 may take the other mask than float64.
The seeds below were chosen on the CPU so that the float64 pre-ReLU value nearest to 0 (`kink`, printed) is at least 1e-6 away in
every case: several float32 roundings of a value of order 1."""
import functools

import pytest
import torch

from rlx_amd.hip import lib as L
from test_gpu_hyper_net import check

#        M, in_dim, hidden, n_blocks, out_dim
CASES = [(1, 17, 64, 1, 0), (33, 23, 512, 2, 100), (128, 40, 1024, 1, 1), (4096, 23, 256, 2, 100)]
FUSED = [(M, *c[1:]) for c in CASES[:3] for M in (1, 33, 128, 257)]
SEEDS = {(4096, 23, 256, 2, 100): 4}      # case -> seed where the default (M + hidden) leaves a pre-ReLU value within 1e-6 of 0
LN_EPS = 1e-6


def layout(in_dim, H, blocks, out_dim):
    """the flat layout (include/rlx_hip.h): [(name, shape)]"""
    vec = lambda p, names: [(p + n, (H,)) for n in names]
    lay = [("W0", (in_dim, H))] + vec("", ("b0", "g0", "be0"))
    for b in range(blocks):
        lay += [(f"{b}.Wa", (H, H))] + vec(f"{b}.", ("ba", "ga", "bea")) + [(f"{b}.Wb", (H, H))] + vec(f"{b}.", ("bb", "gb", "beb"))
    return lay + ([("Wo", (H, out_dim)), ("bo", (out_dim,))] if out_dim else [])


def split(p, *dims):
    w, off = {}, 0
    for name, shape in layout(*dims):
        n = shape[0] * (shape[1] if len(shape) == 2 else 1)
        w[name], off = p[off:off + n].reshape(shape), off + n
    assert off == p.numel()
    return w


def ref_net(c, dt, params, x, d_out):
    """-> dict(out, dx, grads, kink) in dtype dt on the CPU; kink: the pre-ReLU value nearest to 0"""
    M, in_dim, H, blocks, out_dim = c
    p, x = params.to(dt).clone().requires_grad_(), x.to(dt).clone().requires_grad_()
    w = split(p, *c[1:])
    pre = []

    def ln(z, g, b):      # flax's fast variance
        mean = z.mean(-1, keepdim=True)
        var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
        return (z - mean) * torch.rsqrt(var + LN_EPS) * g + b

    def relu(y):
        pre.append(float(y.detach().abs().min()))
        return torch.relu(y)

    h = relu(ln(x @ w["W0"] + w["b0"], w["g0"], w["be0"]))
    for b in range(blocks):
        y = relu(ln(h @ w[f"{b}.Wa"] + w[f"{b}.ba"], w[f"{b}.ga"], w[f"{b}.bea"]))
        h = ln(y @ w[f"{b}.Wb"] + w[f"{b}.bb"], w[f"{b}.gb"], w[f"{b}.beb"]) + h
    out = h @ w["Wo"] + w["bo"] if out_dim else h
    out.backward(d_out.to(dt))
    return dict(out=out.detach(), dx=x.grad, grads=p.grad, kink=min(pre))


@functools.lru_cache(maxsize=None)
def case(c):
    M, in_dim, H, blocks, out_dim = c
    g = torch.Generator().manual_seed(SEEDS.get(c, M + H))
    parts = []
    for name, shape in layout(*c[1:]):
        kind = name.split(".")[-1]
        if len(shape) == 2:      # variance-preserving Dense kernels
            w = torch.randn(shape, generator=g) * (2.0 / shape[0]) ** 0.5
        else:                    # LayerNorm scales 1 +- 10 %, every bias +- 0.1
            w = (1.0 if kind.startswith("g") else 0.0) + 0.1 * (2 * torch.rand(shape, generator=g) - 1)
        parts.append(w.reshape(-1))
    inp = (torch.cat(parts), torch.randn(M, in_dim, generator=g), torch.randn(M, out_dim or H, generator=g))
    return inp, ref_net(c, torch.float64, *inp), ref_net(c, torch.float32, *inp)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_out_dx_and_every_gradient_tensor_match_float64(ctx, dev, c):
    M, in_dim, H, blocks, out_dim = c
    (params, x, d_out), r64, r32 = case(c)
    print(f"{c}: kink {r64['kink']:.3e}")
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, grads, dx = nan(M, out_dim or H), nan(params.numel()), nan(M, in_dim)
    ctx.bro_net(L.bro_desc(in_dim, H, blocks, out_dim), params.to(dev), x.to(dev), out, d_out.to(dev), grads, dx)
    worst = max(check(c, "out", out.cpu(), r64["out"], r32["out"]), check(c, "dx", dx.cpu(), r64["dx"], r32["dx"]))
    g, g64, g32 = (split(t, *c[1:]) for t in (grads.cpu(), r64["grads"], r32["grads"]))
    for name in g:
        worst = max(worst, check(c, name, g[name], g64[name], g32[name]))
    print(f"{c}: worst fraction of a bar {worst:.3f}")


def forward(ctx, dev, c, path):
    (params, x, _), r64, r32 = case(c)
    out = torch.full((c[0], c[4] or c[2]), float("nan"), device=dev)
    ctx.bro_net(L.bro_desc(*c[1:], fwd_path=path), params.to(dev), x.to(dev), out)
    return out.cpu(), r64["out"], r32["out"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", FUSED, ids=str)
def test_the_fused_forward_matches_float64(ctx, dev, c):
    check(c, "out (fused)", *forward(ctx, dev, c, 2))


@pytest.mark.gpu
def test_the_two_forward_routes_agree_within_the_sum_of_their_bars(ctx, dev):
    (o1, e64, e32), (o2, _, _) = forward(ctx, dev, CASES[1], 1), forward(ctx, dev, CASES[1], 2)
    bar = 8 * max(float((e32.double() - e64).abs().max()), 2.0 ** -24 * float(e64.abs().max()))
    assert float((o1 - o2).abs().max()) <= 2 * bar


@pytest.mark.gpu
def test_fused_with_a_backward_is_einval_and_an_odd_width_is_eunsup(ctx, dev):
    c = CASES[0]
    (params, x, d_out), _, _ = case(c)
    out, grads = torch.full((c[0], c[2]), float("nan"), device=dev), torch.full((params.numel(),), float("nan"), device=dev)
    with pytest.raises(L.RlxError, match=r"rc=-1"):       # RLX_EINVAL
        ctx.bro_net(L.bro_desc(*c[1:], fwd_path=2), params.to(dev), x.to(dev), out, d_out.to(dev), grads)
    with pytest.raises(L.RlxError, match=r"rc=-4.*hidden"):       # RLX_EUNSUP names the field
        ctx.bro_net(L.bro_desc(c[1], 96, c[3], c[4]), params.to(dev), x.to(dev), out)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(grads).all())      # nothing was written


def test_param_count_is_the_sum_of_the_layout():
    for dims in ((23, 512, 2, 100), (3, 64, 4, 0)):
        want = sum(s[0] * (s[1] if len(s) == 2 else 1) for _, s in layout(*dims))
        assert L.bro_param_count(L.bro_desc(*dims)) == want
    assert L.bro_param_count(L.bro_desc(17, 0, 2, 0)) == -1
