"""GPU: rlx_cnn_net_f32 (cnn_net.h on cnn.hip) -- out and every gradient tensor of the flat layout, per tensor -- against the torso
written as a plain torch function on the CPU in float64 (tests/test_gpu_conv2d.py's block, autograd for the backward).  A tensor's
bar is tests/test_gpu_hyper_net.py's: 8 x max(the same function's float32 deviation from float64, 2^-24 max |tensor|).

Cases (M, in_c, in_h, in_w, convolutions, hidden, out_dim, norm): (1, 4, 36, 36, reference) the maps shrink 8 -> 3 -> 1, the smallest
input that passes all three layers; (3, 4, 84, 84, reference, 512, 306) the reference shape with a 6-action x 51-atom head; the same
with 6 outputs under pqn's LayerNorms; (130, 1, 20, 16, two layers, 128, 1) non-square, and the weight gradient in many slabs: the
library takes min(M, CUs / K tiles) slabs of ceil(M / that) images, a K tile being 128 rows of the k k ci axis.  The first layer has
16 rows (one tile), the second 288 (three), so with 256 CUs that is 130 slabs of one image and 65 slabs of two; at least two slabs
on any device with two CUs or more.  (4096, 1, 4, 3, one layer, 64, 2) with d_out of order 1 / M, a mean loss's: the row count from
which the tree's weight-gradient launcher would move to the split-operand fp16 engine by itself (an absolute floor of 2^-25 on the
gradient operand, far above this bar at such a d_out); the torso must stay exact fp32 there.

The seeds (default M + hidden; SEEDS lists the others) keep the float64 pre-ReLU value nearest to 0 at least 1e-6 away."""
import functools

import pytest
import torch

from rlx_amd.hip import lib as L
from test_gpu_conv2d import LN_EPS, conv_block, ln
from test_gpu_hyper_net import check

REF = ((32, 8, 4), (64, 4, 2), (64, 3, 1))
CASES = [(1, 4, 36, 36, REF, 64, 3, 0), (3, 4, 84, 84, REF, 512, 306, 0), (2, 4, 84, 84, REF, 512, 6, 1),
         (130, 1, 20, 16, ((32, 4, 2), (64, 3, 1)), 128, 1, 1), (4096, 1, 4, 3, ((32, 3, 1),), 64, 2, 0)]
SEEDS = {CASES[3]: 1}      # case -> seed where the default leaves a pre-ReLU value within 1e-6 of 0 (there: 2.4e-7)


def desc(c):
    M, in_c, in_h, in_w, convs, hidden, out_dim, norm = c
    return L.cnn_desc(out_dim, in_c, in_h, in_w, convs, hidden, norm, LN_EPS)


def layout(in_c, in_h, in_w, convs, hidden, out_dim, norm):
    """the flat layout (include/rlx_hip.h): [(name, shape)]"""
    lay, ci, h, w = [], in_c, in_h, in_w
    for l, (co, k, s) in enumerate(convs):
        lay += [(f"{l}.W", (k, k, ci, co)), (f"{l}.b", (co,))] + ([(f"{l}.g", (co,)), (f"{l}.be", (co,))] if norm else [])
        ci, h, w = co, (h - k) // s + 1, (w - k) // s + 1
    lay += [("Wd", (h * w * ci, hidden)), ("bd", (hidden,))] + ([("gd", (hidden,)), ("bed", (hidden,))] if norm else [])
    return lay + [("Wo", (hidden, out_dim)), ("bo", (out_dim,))]


def split(p, *dims):
    w, off = {}, 0
    for name, shape in layout(*dims):
        n = torch.Size(shape).numel()
        w[name], off = p[off:off + n].reshape(shape), off + n
    assert off == p.numel()
    return w


def ref_net(c, dt, params, x, d_out):
    """-> dict(out, grads, kink) in dtype dt on the CPU; kink: the pre-ReLU value nearest to 0"""
    convs, norm = c[4], c[7]
    p = params.to(dt).clone().requires_grad_()
    w = split(p, *c[1:])
    kink, h = [], (x.to(dt) / 255)
    for l, (co, k, s) in enumerate(convs):
        y, pre = conv_block(h, w[f"{l}.W"], w[f"{l}.b"], w.get(f"{l}.g"), w.get(f"{l}.be"), s)
        kink.append(float(pre.detach().abs().min()))
        h = y.permute(0, 3, 1, 2)
    zd = y.reshape(y.shape[0], -1) @ w["Wd"] + w["bd"]
    pre = ln(zd, w["gd"], w["bed"]) if norm else zd
    kink.append(float(pre.detach().abs().min()))
    out = torch.relu(pre) @ w["Wo"] + w["bo"]
    out.backward(d_out.to(dt))
    return dict(out=out.detach(), grads=p.grad, kink=min(kink))


@functools.lru_cache(maxsize=None)
def case(c):
    M, in_c, in_h, in_w, convs, hidden, out_dim, norm = c
    g = torch.Generator().manual_seed(SEEDS.get(c, M + hidden))
    parts = []
    for name, shape in layout(*c[1:]):
        if len(shape) > 1:      # variance-preserving kernels
            w = torch.randn(shape, generator=g) * (2.0 / torch.Size(shape[:-1]).numel()) ** 0.5
        else:                   # LayerNorm scales 1 +- 10 %, every bias +- 0.1
            w = (1.0 if name.split(".")[-1].startswith("g") else 0.0) + 0.1 * (2 * torch.rand(shape, generator=g) - 1)
        parts.append(w.reshape(-1))
    inp = (torch.cat(parts), torch.randint(0, 256, (M, in_c, in_h, in_w), generator=g, dtype=torch.uint8), torch.randn(M, out_dim, generator=g) / (M if M >= 4096 else 1))
    return inp, ref_net(c, torch.float64, *inp), ref_net(c, torch.float32, *inp)


def run(ctx, dev, c):
    (params, x, d_out), _, _ = case(c)
    out, grads = torch.full((c[0], c[6]), float("nan"), device=dev), torch.full((params.numel(),), float("nan"), device=dev)
    ctx.cnn_net(desc(c), params.to(dev), x.to(dev), out, d_out.to(dev), grads)
    return out.cpu(), grads.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_out_and_every_gradient_tensor_match_float64(ctx, dev, c):
    _, r64, r32 = case(c)
    print(f"{c}: kink {r64['kink']:.3e}")
    assert r64["kink"] >= 1e-6
    out, grads = run(ctx, dev, c)
    worst = check(c, "out", out, r64["out"], r32["out"])
    g, g64, g32 = (split(t, *c[1:]) for t in (grads, r64["grads"], r32["grads"]))
    for name in g:
        worst = max(worst, check(c, name, g[name], g64[name], g32[name]))
    print(f"{c}: worst fraction of a bar {worst:.3f}")


@pytest.mark.gpu
def test_identical_calls_give_identical_bits(ctx, dev):
    (o1, g1), (o2, g2) = run(ctx, dev, CASES[1]), run(ctx, dev, CASES[1])
    assert torch.equal(o1, o2) and torch.equal(g1, g2)


@pytest.mark.gpu
@pytest.mark.parametrize("convs, in_hw, field", [(((48, 8, 4), (64, 4, 2), (64, 3, 1)), 36, r"ch \(output channels\)"), (REF, 20, "kernel is larger")])
def test_outside_the_envelope_is_eunsup_and_writes_nothing(ctx, dev, convs, in_hw, field):
    c = (1, 4, in_hw, in_hw, convs, 64, 3, 0)
    out, grads = torch.full((1, 3), float("nan"), device=dev), torch.full((200000,), float("nan"), device=dev)
    with pytest.raises(L.RlxError, match=rf"rc=-4.*{field}"):       # RLX_EUNSUP names the field
        ctx.cnn_net(desc(c), torch.zeros(200000, device=dev), torch.zeros(1, 4, in_hw, in_hw, dtype=torch.uint8, device=dev), out,
                    torch.zeros(1, 3, device=dev), grads)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(grads).all())


def test_param_count_is_the_sum_of_the_layout():
    for c in CASES:
        assert L.cnn_param_count(desc(c)) == sum(torch.Size(s).numel() for _, s in layout(*c[1:]))
    assert L.cnn_param_count(L.cnn_desc(6, hidden=0)) == -1
