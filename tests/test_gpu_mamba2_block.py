"""GPU: rlx_mamba2_f32 (mamba2_block.h on ssm.hip) -- out, hT, convT, dx and every parameter gradient, per tensor of the flat layout --
against the float64 token loop of tests/test_gpu_ssm_scan.py (its ssm_core, place_done and bar) extended by the block's formulas:
u0 | z = ln(x) W_in + b_in;  dt_raw | B | C = u W_x + b_x;  x += g W_out + b_out.  The CPU test at the bottom checks
rlx_mamba2_param_count.

The last case has exactly 4096 rows: its GEMMs run on the split-operand engine (fp32 operands split exactly into fp16 pieces on the
matrix pipe), the others on the exact engine."""
import functools

import pytest
import torch
import torch.nn.functional as F

from rlx_amd.hip import lib as L
from test_gpu_ssm_scan import place_done, ssm_core

#        S, T, d_model, expand, N, K, layers
CASES = [(3, 37, 64, 2, 8, 4, 1), (2, 20, 128, 2, 8, 4, 2), (2, 1, 64, 2, 8, 4, 2), (32, 128, 64, 2, 8, 4, 1)]
EPS = 1e-5


def layout(d, I, N, K, layers):
    """the flat layout (include/rlx_hip.h): [(name, shape)]"""
    per = [("ln_scale", (d,)), ("ln_bias", (d,)), ("W_in", (d, 2 * I)), ("b_in", (2 * I,)), ("conv_w", (K, I)), ("conv_b", (I,)),
           ("W_x", (I, I + 2 * N)), ("b_x", (I + 2 * N,)), ("dt_bias", (I,)), ("A_log", (I, N)), ("D", (I,)), ("W_out", (I, d)), ("b_out", (d,))]
    return [(f"{l}.{n}", s) for l in range(layers) for n, s in per]


def ref_block(c, dt, done, params, x, h0, c0, d_out):
    """-> dict(out, hT, convT, dx, grads) in dtype dt on the CPU"""
    S, T, d, ex, N, K, layers = c
    I = d * ex
    p = params.to(dt).clone().requires_grad_()
    x = x.to(dt).clone().requires_grad_()
    h, off, hT, cT = x, 0, [], []
    for l in range(layers):
        w = {}
        for name, shape in layout(d, I, N, K, 1):
            n = int(torch.tensor(shape).prod())
            w[name[2:]], off = p[off:off + n].reshape(shape), off + n
        proj = (F.layer_norm(h, (d,), w["ln_scale"], w["ln_bias"], EPS) @ w["W_in"] + w["b_in"]).reshape(S, T, 2 * I)
        u0, z = proj[..., :I], proj[..., I:]
        # (the x_proj GEMM reads u, the conv's output: run the loop once for u, then again with dt_raw | B | C in place)
        us, _, _, _ = ssm_core(done, u0, z, u0, u0[..., :N], u0[..., :N], w["conv_w"], w["conv_b"], w["A_log"], w["D"], w["dt_bias"],
                               h0[:, l].to(dt), c0[:, l].to(dt))
        xp = torch.stack(us, 1) @ w["W_x"] + w["b_x"]
        _, g, hl, cl = ssm_core(done, u0, z, xp[..., :I], xp[..., I:I + N], xp[..., I + N:], w["conv_w"], w["conv_b"], w["A_log"], w["D"],
                                w["dt_bias"], h0[:, l].to(dt), c0[:, l].to(dt))
        h = h + g.reshape(S * T, I) @ w["W_out"] + w["b_out"]
        hT.append(hl)
        cT.append(cl)
    out = dict(out=h.detach(), hT=torch.stack(hT, 1).detach(), convT=torch.stack(cT, 1).detach())
    if d_out is not None:
        h.backward(d_out.to(dt))
        out.update(dx=x.grad, grads=p.grad)
    return out


@functools.lru_cache(maxsize=None)
def case(c):
    S, T, d, ex, N, K, layers = c
    I = d * ex
    g = torch.Generator().manual_seed(d + T)
    parts = []
    for name, shape in layout(d, I, N, K, layers):
        w = torch.randn(shape, generator=g)
        kind = name[2:]
        if kind == "A_log":
            w = torch.log(torch.arange(1, N + 1.0))[None] + 0.1 * w
        elif kind == "dt_bias":
            w = torch.log(torch.expm1(torch.exp(torch.empty(I).uniform_(-6.9, -2.3, generator=g))))
        elif kind in ("ln_scale", "D"):
            w = 1 + 0.1 * w
        elif kind == "conv_w":
            w = 0.5 * w
        else:
            w = 0.1 * w if len(shape) == 1 else w / shape[0] ** 0.5
        parts.append(w.reshape(-1))
    r = lambda *s: torch.randn(*s, generator=g)
    bwd = T > 1       # the acting step is forward only
    inp = (place_done(S, T), torch.cat(parts), r(S * T, d), r(S, layers, I, N), r(S, layers, K - 1, I), r(S * T, d) if bwd else None)
    return inp, ref_block(c, torch.float64, *inp), ref_block(c, torch.float32, *inp)


def run(ctx, dev, c):
    S, T, d, ex, N, K, layers = c
    I = d * ex
    (done, params, x, h0, c0, d_out), _, _ = case(c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out = dict(out=nan(S * T, d), hT=nan(S, layers, I, N), convT=nan(S, layers, K - 1, I))
    kw = dict(d_out=d_out.to(dev), grads=nan(params.numel()), dx=nan(S * T, d)) if d_out is not None else {}
    ctx.mamba2(L.mamba2_desc(d, ex, N, K, layers, EPS), params.to(dev), x.to(dev), torch.from_numpy(done).to(dev), out["out"], h0.to(dev),
               c0.to(dev), out["hT"], out["convT"], **kw)
    return {k: v.cpu() for k, v in dict(out, **{k: v for k, v in kw.items() if k != "d_out"}).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_outputs_carries_dx_and_parameter_gradients_match_float64(ctx, dev, c):
    """bar per tensor: 8 x max(the float32 reference's deviation from float64, 2^-24 max |tensor|), on both engines"""
    S, T, d, ex, N, K, layers = c
    _, r64, r32 = case(c)
    got = run(ctx, dev, c)
    tensors = [(k, slice(None)) for k in got if k != "grads"]
    if "grads" in got:
        off = 0
        for name, shape in layout(d, d * ex, N, K, layers):
            n = int(torch.tensor(shape).prod())
            tensors.append((name, slice(off, off + n)))
            off += n
        assert off == got["grads"].numel()
    worst = 0.0
    for name, sl in tensors:
        k = name if name in got else "grads"
        a, e64, e32 = got[k].reshape(-1)[sl].double(), r64[k].reshape(-1)[sl], r32[k].reshape(-1)[sl].double()
        bar = 8 * max(float((e32 - e64).abs().max()), 2.0 ** -24 * float(e64.abs().max()))
        err = float((a - e64).abs().max())
        worst = max(worst, err / bar)
        print(f"{c} {name}: max error {err:.3e}, bar {bar:.3e}, fraction {err / bar:.3f}")
        assert err <= bar, (name, err, bar)
    print(f"{c}: worst fraction of a bar {worst:.3f}")


def test_param_count_is_the_sum_of_the_layout():
    for d, ex, N, K, layers in ((128, 2, 8, 4, 1), (64, 3, 16, 2, 4)):
        want = sum(int(torch.tensor(s).prod()) for _, s in layout(d, d * ex, N, K, layers))
        assert L.mamba2_param_count(L.mamba2_desc(d, ex, N, K, layers)) == want
