"""GPU: rlx_tf_encoder_f32 (tf_encoder.h on attn.hip) -- out, dx and every parameter gradient, per tensor of the flat layout --
against the same float64 reference as tests/test_gpu_band_attn.py (its masks, mask and bar), extended by the layer's formulas:
x += Wo attn(ln1(x) Wqkv + bqkv) + bo;  x += W2 relu(W1 ln2(x) + b1) + b2.  The CPU test at the bottom checks rlx_tf_param_count."""
import functools

import pytest
import torch
import torch.nn.functional as F

from rlx_amd.hip import lib as L
from test_gpu_band_attn import keep_mask, masks

#        d_model, nhead, ff, layers, C, S, T
CASES = [(128, 4, 512, 2, 16, 3, 37), (64, 1, 128, 1, 3, 2, 16), (256, 8, 256, 3, 16, 1, 21)]


def layout(d, ff, layers):
    """the flat layout (include/rlx_hip.h): [(name, shape)]"""
    per = [("ln1_scale", (d,)), ("ln1_bias", (d,)), ("Wqkv", (d, 3 * d)), ("bqkv", (3 * d,)), ("Wo", (d, d)), ("bo", (d,)),
           ("ln2_scale", (d,)), ("ln2_bias", (d,)), ("W1", (d, ff)), ("b1", (ff,)), ("W2", (ff, d)), ("b2", (d,))]
    return [(f"{l}.{n}", s) for l in range(layers) for n, s in per]


def ref_encoder(params, x, keep, c, dtype, d_out):
    """-> out, dx, flat grads in dtype on the CPU"""
    d, nhead, ff, layers, C, S, T = c
    p = params.to(dtype).clone().requires_grad_()      # (clone: .to() of the same dtype returns the cached input itself)
    x = x.to(dtype).clone().requires_grad_()
    h, off, eps = x, 0, 1e-5
    for name, shape in layout(d, ff, layers):
        n = int(torch.tensor(shape).prod())
        w, off = p[off:off + n].reshape(shape), off + n
        kind = name.split(".")[1]
        if kind in ("ln1_scale", "ln2_scale"):
            scale = w
        elif kind in ("ln1_bias", "ln2_bias"):
            y = F.layer_norm(h, (d,), scale, w, eps)
        elif kind in ("Wqkv", "Wo", "W1", "W2"):
            W = w
        elif kind == "bqkv":
            q, k, v = ((y @ W + w).reshape(S, T, 3, nhead, d // nhead)[:, :, i] for i in range(3))
            logits = torch.einsum("sihd,sjhd->shij", q * (d // nhead) ** -0.5, k)
            logits = torch.where(keep[:, None], logits, torch.finfo(dtype).min)
            y = torch.einsum("shij,sjhd->sihd", torch.softmax(logits, -1), v).reshape(S * T, d)
        elif kind == "b1":
            y = torch.relu(y @ W + w)
        else:       # bo, b2: the branch closes on its residual
            h = h + y @ W + w
    h.backward(d_out.to(dtype))
    return h.detach(), x.grad, p.grad


@functools.lru_cache(maxsize=None)
def case(c):
    d, nhead, ff, layers, C, S, T = c
    g = torch.Generator().manual_seed(d + T)
    seg, valid = masks(S, T, C)
    keep = torch.from_numpy(keep_mask(seg, valid, C)[0])
    rows = torch.from_numpy(valid.reshape(-1).astype(bool))
    parts = []
    for name, shape in layout(d, ff, layers):
        w = torch.randn(shape, generator=g)
        parts.append((1 + 0.1 * w if "scale" in name else 0.1 * w if len(shape) == 1 else w / shape[0] ** 0.5).reshape(-1))
    params, x = torch.cat(parts), torch.randn(S * T, d, generator=g)
    d_out = torch.randn(S * T, d, generator=g) * rows[:, None]
    return seg, valid, rows, keep, params, x, d_out


def run(ctx, dev, c, d_out, dropout=0.0):
    d, nhead, ff, layers, C, S, T = c
    seg, valid, rows, keep, params, x, _ = case(c)
    out, dx, grads = (torch.full(s, float("nan"), device=dev) for s in ((S * T, d), (S * T, d), (params.numel(),)))
    ctx.tf_encoder(L.tf_desc(d, nhead, ff, layers, C, 1e-5, dropout), params.to(dev), x.to(dev), torch.from_numpy(seg).to(dev),
                   torch.from_numpy(valid).to(dev), out, d_out.to(dev), grads, dx)
    return out.cpu(), dx.cpu(), grads.cpu()


def compare(c, got, d_out_ref):
    """every tensor within 8 x the float32 reference's own deviation from float64; dx exactly 0 at invalid rows"""
    d, nhead, ff, layers = c[:4]
    seg, valid, rows, keep, params, x, _ = case(c)
    r64 = ref_encoder(params, x, keep, c, torch.float64, d_out_ref)
    r32 = ref_encoder(params, x, keep, c, torch.float32, d_out_ref)
    worst = 0.0
    for i, name in enumerate(("out", "dx")):
        bar = 8 * float((r32[i].double() - r64[i])[rows].abs().max())
        err = float((got[i].double() - r64[i])[rows].abs().max())
        worst = max(worst, err / max(bar, 1e-300))
        assert err <= bar, (name, err, bar)
    off = 0
    for name, shape in layout(d, ff, layers):
        n = int(torch.tensor(shape).prod())
        bar = 8 * float((r32[2][off:off + n].double() - r64[2][off:off + n]).abs().max())
        err = float((got[2][off:off + n].double() - r64[2][off:off + n]).abs().max())
        worst = max(worst, err / max(bar, 1e-300))
        assert err <= bar, (name, err, bar)
        off += n
    print(f"{c}: worst fraction of a bar {worst:.3f}")
    assert torch.all(got[1][~rows] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_out_dx_and_parameter_gradients_match_float64(ctx, dev, c):
    compare(c, run(ctx, dev, c, case(c)[6]), case(c)[6])


@pytest.mark.gpu
def test_an_invalid_token_contributes_nothing(ctx, dev):
    """d_out is 0 at all valid rows but one; the library is also handed junk at the invalid rows, the reference zeros there"""
    c = CASES[0]
    rows, d_out = case(c)[2], case(c)[6]
    one = torch.zeros_like(d_out)
    one[20] = d_out[20]
    assert rows[20] and (~rows).any()
    junk = one.clone()
    junk[~rows] = 3.0
    compare(c, run(ctx, dev, c, junk), one)


@pytest.mark.gpu
@pytest.mark.parametrize("c, dropout", [(CASES[1], 0.1), ((96, 1, 128, 1, 3, 2, 16), 0.0)], ids=["dropout", "d_model96"])
def test_refusals(ctx, dev, c, dropout):
    d, S, T = c[0], c[5], c[6]
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    with pytest.raises(L.RlxError, match=r"rc=-4"):       # RLX_EUNSUP
        ctx.tf_encoder(L.tf_desc(d, c[1], c[2], c[3], c[4], 1e-5, dropout), z(L.tf_param_count(L.tf_desc(d, c[1], c[2], c[3]))),
                       z(S * T, d), z(S, T, dt=torch.int32), z(S, T, dt=torch.uint8), z(S * T, d))


def test_param_count_is_the_sum_of_the_layout():
    for d, nhead, ff, layers in ((128, 4, 512, 2), (64, 1, 100, 3)):
        want = sum(int(torch.tensor(s).prod()) for _, s in layout(d, ff, layers))
        assert L.tf_param_count(L.tf_desc(d, nhead, ff, layers)) == want
