"""GPU: rlx_hyper_net_f32 (hyper_net.h on hyper.hip) -- out, dx and every gradient tensor of the flat layout, per tensor -- against the
formulas of include/rlx_hip.h's section written as a plain torch function on the CPU in float64 (autograd for the backward).  A
tensor's bar is 8 x max(the same function's float32 deviation from float64, 2^-24 max |tensor|): tests/test_gpu_ssm_scan.py's formula,
computed from the reference alone.  The CPU test at the bottom checks rlx_hyper_param_count.

(5, 11, 64, 1): M no multiple of a workgroup's four rows.  (37, 22, 128, 2): in + 1 = 23 is odd (the padded stride) and two blocks
(the residual path).  (256, 17, 512, 2): the reference critic's widths, X = 2048.  (4096, 8, 64, 1): the split-operand engine."""
import functools

import pytest
import torch

from rlx_amd.hip import lib as L

#        M, in_dim, hidden, n_blocks      (expansion 4, the reference's constants: lib.hyper_desc's defaults)
CASES = [(5, 11, 64, 1), (37, 22, 128, 2), (256, 17, 512, 2), (4096, 8, 64, 1)]
EX, EPS = 4, 1e-8


def layout(in_dim, H, blocks):
    """the flat layout (include/rlx_hip.h): [(name, shape)]"""
    per = [("W1", (H, EX * H)), ("s1", (EX * H,)), ("W2", (EX * H, H)), ("a", (H,))]
    return [("W_e", (in_dim + 1, H)), ("s_e", (H,))] + [(f"{b}.{n}", s) for b in range(blocks) for n, s in per]


def split(p, in_dim, H, blocks):
    w, off = {}, 0
    for name, shape in layout(in_dim, H, blocks):
        n = shape[0] * (shape[1] if len(shape) == 2 else 1)
        w[name], off = p[off:off + n].reshape(shape), off + n
    assert off == p.numel()
    return w


def l2n(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(EPS)


def ref_net(c, dt, desc, params, x, d_out):
    """-> dict(out [, dx, grads]) in dtype dt on the CPU"""
    M, in_dim, H, blocks = c
    cs, ca = desc.scaler_init / desc.scaler_scale, desc.alpha_init / desc.alpha_scale
    p, x = params.to(dt).clone().requires_grad_(), x.to(dt).clone().requires_grad_()
    w = split(p, in_dim, H, blocks)
    h = l2n(w["s_e"] * (cs * (l2n(torch.cat([x, torch.full((M, 1), desc.c_shift, dtype=dt)], 1)) @ w["W_e"])))
    for b in range(blocks):
        y = l2n((torch.relu(w[f"{b}.s1"] * (cs * (h @ w[f"{b}.W1"]))) + EPS) @ w[f"{b}.W2"])
        h = l2n(h + w[f"{b}.a"] * (ca * (y - h)))
    if d_out is None:
        return dict(out=h.detach())
    h.backward(d_out.to(dt))
    return dict(out=h.detach(), dx=x.grad, grads=p.grad)


@functools.lru_cache(maxsize=None)
def case(c, zero_w2=False):
    M, in_dim, H, blocks = c
    desc = L.hyper_desc(in_dim, H, blocks, EX)
    g = torch.Generator().manual_seed(M + H)
    parts = []
    for name, shape in layout(in_dim, H, blocks):
        if len(shape) == 2:      # random, then projected to unit columns in float64
            w = torch.randn(shape, generator=g, dtype=torch.float64)
            w = (w / w.norm(dim=0, keepdim=True).clamp_min(EPS)).float()
            if zero_w2 and name == "0.W2":
                w = torch.zeros(shape)
        else:                    # Scalers and alphas: their initial value +- 10 %
            init = {"s_e": desc.scaler_scale, "s1": desc.scaler_scale / EX ** 0.5, "a": desc.alpha_scale}[name.split(".")[-1]]
            w = init * (1 + 0.1 * (2 * torch.rand(shape, generator=g) - 1))
        parts.append(w.reshape(-1))
    inp = (desc, torch.cat(parts), torch.randn(M, in_dim, generator=g), None if zero_w2 else torch.randn(M, H, generator=g))
    return inp, ref_net(c, torch.float64, *inp), ref_net(c, torch.float32, *inp)


def check(c, name, a, e64, e32):
    """-> the error's fraction of the bar"""
    bar = 8 * max(float((e32.double() - e64).abs().max()), 2.0 ** -24 * float(e64.abs().max()))
    err = float((a.double() - e64).abs().max())
    print(f"{c} {name}: max error {err:.3e}, bar {bar:.3e}, fraction {err / bar:.3f}")
    assert err <= bar, (name, err, bar)
    return err / bar


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_out_dx_and_every_gradient_tensor_match_float64(ctx, dev, c):
    M, in_dim, H, blocks = c
    (desc, params, x, d_out), r64, r32 = case(c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, grads, dx = nan(M, H), nan(params.numel()), nan(M, in_dim)
    ctx.hyper_net(desc, params.to(dev), x.to(dev), out, d_out.to(dev), grads, dx)
    worst = max(check(c, "out", out.cpu(), r64["out"], r32["out"]), check(c, "dx", dx.cpu(), r64["dx"], r32["dx"]))
    g, g64, g32 = (split(t, in_dim, H, blocks) for t in (grads.cpu(), r64["grads"], r32["grads"]))
    for name in g:
        worst = max(worst, check(c, name, g[name], g64[name], g32[name]))
    print(f"{c}: worst fraction of a bar {worst:.3f}")


@pytest.mark.gpu
def test_a_zero_w2_takes_the_clamp_branch_forward(ctx, dev):
    """z2 = 0 in block 0: the clamped norm gives y = 0 and out must meet its bar (forward only; no dx, no grads)"""
    c = CASES[1]
    (desc, params, x, _), r64, r32 = case(c, True)
    out = torch.full((c[0], c[2]), float("nan"), device=dev)
    ctx.hyper_net(desc, params.to(dev), x.to(dev), out)
    check(c, "out", out.cpu(), r64["out"], r32["out"])


def test_param_count_is_the_sum_of_the_layout():
    for in_dim, H, blocks in ((17, 512, 2), (3, 64, 4)):
        want = sum(s[0] * (s[1] if len(s) == 2 else 1) for _, s in layout(in_dim, H, blocks))
        assert L.hyper_param_count(L.hyper_desc(in_dim, H, blocks, EX)) == want
    assert L.hyper_param_count(L.hyper_desc(17, 0, 2, EX)) == -1
