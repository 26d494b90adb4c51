"""GPU: rlx_conv2d_f32 (cnn.hip) -- y, dx (float32 input), gW, gb and, with norm, g_gbe -- against torch.nn.functional.conv2d on the
CPU in float64 (autograd for the backward), the LayerNorm written out with flax's fast variance.  A tensor's bar is
tests/test_gpu_hyper_net.py's: 8 x max(the same function's float32 deviation from float64, 2^-24 max |tensor|).

Cases (M, CI, H, W, kernel, stride, CO, uint8 input, norm): (1, 4, 12, 12, 8, 4, 32) four output pixels, one image; (3, 1, 13, 10, 3, 1,
64) one channel (padded to a pair), non-square, odd image count; (2, 32, 11, 9, 4, 2, 64) 4 x 3 pixels, input row 10 and column 8 are
never read, so dx there must be exactly 0 -- without and with the channel LayerNorm; (5, 4, 84, 84, 8, 4, 32) the reference's first
layer, four bands of 100 pixels, odd M; (2, 32, 20, 20, 4, 2, 64) its second, 81 pixels; (2, 64, 9, 9, 3, 1, 64) its third, 49.

The ReLU's backward has a kink at 0: the seeds (default M + H + CO; SEEDS lists the others) keep the float64 pre-ReLU value nearest
to 0 at least 1e-6 away, and the test asserts that on the reference."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_hyper_net import check

CASES = [(1, 4, 12, 12, 8, 4, 32, 1, 0), (3, 1, 13, 10, 3, 1, 64, 1, 0), (2, 32, 11, 9, 4, 2, 64, 0, 0), (2, 32, 11, 9, 4, 2, 64, 0, 1),
         (5, 4, 84, 84, 8, 4, 32, 1, 1), (2, 32, 20, 20, 4, 2, 64, 0, 0), (2, 64, 9, 9, 3, 1, 64, 0, 0)]
SEEDS = {}      # case -> seed where the default leaves a pre-ReLU value within 1e-6 of 0
LN_EPS = 1e-6


def ln(z, g, b):      # flax's fast variance, over the last axis
    mean = z.mean(-1, keepdim=True)
    var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    return (z - mean) * torch.rsqrt(var + LN_EPS) * g + b


def conv_block(x_nchw, W, b, g, be, stride):
    """-> (y NHWC, the pre-ReLU values); W is HWIO"""
    z = F.conv2d(x_nchw, W.permute(3, 2, 0, 1), b, stride=stride).permute(0, 2, 3, 1)
    pre = z if g is None else ln(z, g, be)
    return torch.relu(pre), pre


def ref(c, dt, x, W, b, gbe, d_y):
    M, CI, H, Wd, k, s, CO, u8, norm = c
    W, b, gbe = (t.to(dt).clone().requires_grad_() for t in (W, b, gbe))
    xin = x.to(dt) / 255 if u8 else x.to(dt).clone().requires_grad_()
    y, pre = conv_block(xin if u8 else xin.permute(0, 3, 1, 2), W, b, gbe[:CO] if norm else None, gbe[CO:] if norm else None, s)
    y.backward(d_y.to(dt))
    return dict(y=y.detach(), dx=None if u8 else xin.grad, gW=W.grad, gb=b.grad, g_gbe=gbe.grad, kink=float(pre.detach().abs().min()))


@functools.lru_cache(maxsize=None)
def case(c):
    M, CI, H, Wd, k, s, CO, u8, norm = c
    g = torch.Generator().manual_seed(SEEDS.get(c, M + H + CO))
    x = torch.randint(0, 256, (M, CI, H, Wd), generator=g, dtype=torch.uint8) if u8 else torch.randn(M, H, Wd, CI, generator=g)
    W = torch.randn(k, k, CI, CO, generator=g) * (2.0 / (k * k * CI)) ** 0.5
    b = 0.1 * (2 * torch.rand(CO, generator=g) - 1)
    gbe = torch.cat([1 + 0.1 * (2 * torch.rand(CO, generator=g) - 1), 0.1 * (2 * torch.rand(CO, generator=g) - 1)])
    inp = (x, W, b, gbe, torch.randn(M, (H - k) // s + 1, (Wd - k) // s + 1, CO, generator=g))
    return inp, ref(c, torch.float64, *inp), ref(c, torch.float32, *inp)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_y_and_every_gradient_match_float64(ctx, dev, c):
    M, CI, H, Wd, k, s, CO, u8, norm = c
    (x, W, b, gbe, d_y), r64, r32 = case(c)
    print(f"{c}: kink {r64['kink']:.3e}")
    assert r64["kink"] >= 1e-6
    nan = lambda *sh: torch.full(sh, float("nan"), device=dev)
    out = dict(y=nan(*d_y.shape), dx=None if u8 else nan(M, H, Wd, CI), gW=nan(*W.shape), gb=nan(CO), g_gbe=nan(2 * CO) if norm else None)
    ctx.conv2d(x.to(dev), W.to(dev), b.to(dev), s, out["y"], gbe.to(dev) if norm else None, LN_EPS, d_y.to(dev), out["dx"], out["gW"],
               out["gb"], out["g_gbe"])
    worst = max(check(c, name, t.cpu(), r64[name], r32[name]) for name, t in out.items() if t is not None)
    print(f"{c}: worst fraction of a bar {worst:.3f}")
    if (H - k) % s and not u8:      # what VALID padding never reads gets an exact zero
        dx = out["dx"].cpu()
        assert bool((dx[:, (H - k) // s * s + k:] == 0).all()) and bool((dx[:, :, (Wd - k) // s * s + k:] == 0).all())
