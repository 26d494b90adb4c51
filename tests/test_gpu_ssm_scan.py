"""GPU: rlx_ssm_conv_f32 and rlx_ssm_scan_f32 (ssm.hip) against a plain torch-on-CPU loop over tokens written from the formulas in
include/rlx_hip.h -- the window / state entering token t is zeroed where done[s, t - 1], the convolution, SiLU, the selective
recurrence, the z gate -- with autograd, evaluated in float64 and again in float32.

A tensor's bar is 8 x max(largest |float32 reference - float64 reference| on that case, 2^-24 max |float64 tensor|): the project's
margin where only the order of operations differs, over the floor below which float32 cannot resolve the tensor at all.

place_done() puts the episode ends by hand; the tests assert on done what a case is said to contain."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

#        S, T, I, N, K
CASES = [(2, 5, 64, 8, 4), (3, 37, 64, 8, 4), (5, 16, 192, 8, 3), (1, 130, 128, 16, 2), (2, 19, 64, 4, 1), (2, 1, 64, 8, 4)]
RAGGED = CASES[1]


def place_done(S, T):
    """uint8 [S, T]: sequence s ends episodes after tokens 3 + s (inside a chunk), 15 (the reset falls on a chunk start), 19, 25 and
    26 (consecutive), 31 and T - 1 (changes nothing in the call) where those exist; the last of several sequences has none"""
    done = np.zeros((S, T), np.uint8)
    for s in range(S - 1 if S > 1 else S):
        done[s, [p for p in (3 + s, 15, 19, 25, 26, 31, T - 1) if p < T]] = 1
    return done


def ssm_core(done, u0, z, dtr, B, C, w, cb, Alog, D, dtb, h0, c0):
    """the token loop on tensors of one dtype -> u per token, g [S, T, I], hT, convT"""
    h, cs, A, us, gs = h0, c0, -torch.exp(Alog), [], []
    for t in range(u0.shape[1]):
        if t > 0:
            r = torch.from_numpy(1 - done[:, t - 1]).to(u0.dtype)[:, None, None]
            h, cs = h * r, cs * r
        ci = torch.cat([cs, u0[:, t:t + 1]], 1)
        cs = ci[:, 1:]
        u = F.silu((ci * w[None]).sum(1) + cb)
        us.append(u)
        d = F.softplus(dtr[:, t] + dtb)
        h = torch.exp(d[..., None] * A[None]) * h + d[..., None] * B[:, t, None, :] * u[..., None]
        gs.append(((h * C[:, t, None, :]).sum(-1) + D * u) * F.silu(z[:, t]))
    return us, torch.stack(gs, 1), h, cs


def ssm_ref(dt, done, u0, z, dtr, B, C, w, cb, Alog, D, dtb, h0, c0, d_g):
    """ssm_core in dtype dt with autograd under the cotangent d_g -> dict of outputs and gradients"""
    ins = [t.to(dt).clone().requires_grad_() for t in (u0, z, dtr, B, C, w, cb, Alog, D, dtb)]
    us, g, h, cs = ssm_core(done, *ins, h0.to(dt), c0.to(dt))
    for u in us:
        u.retain_grad()
    g.backward(d_g.to(dt))
    names = ("d_u0", "d_z", "d_dtr", "d_B", "d_C", "d_conv_w", "d_conv_b", "d_A_log", "d_D", "d_dt_bias")
    return dict({n: i.grad for n, i in zip(names, ins)}, u=torch.stack(us, 1).detach(), g=g.detach(), hT=h.detach(), convT=cs.detach(),
                d_u=torch.stack([u.grad for u in us], 1))


def bars(r64, r32):
    return {k: 8 * max(float((r32[k].double() - r64[k]).abs().max()), 2.0 ** -24 * float(r64[k].abs().max())) for k in r64 if r64[k].numel()}


@functools.lru_cache(maxsize=None)
def case(c):
    """inputs, the float64 reference and the bars of a case, built once"""
    S, T, I, N, K = c
    g = torch.Generator().manual_seed(100 * S + T)
    r = lambda *s: torch.randn(*s, generator=g)
    done = place_done(S, T)
    dtb = torch.exp(torch.empty(I).uniform_(np.log(1e-3), np.log(1e-1), generator=g))       # the reference's dt initialiser range
    inp = dict(u0=r(S, T, I), z=r(S, T, I), dtr=r(S, T, I), B=r(S, T, N), C=r(S, T, N), w=0.5 * r(K, I), cb=0.1 * r(I),
               Alog=torch.log(torch.arange(1, N + 1.0))[None].repeat(I, 1) + 0.1 * r(I, N), D=1 + 0.1 * r(I),
               dtb=torch.log(torch.expm1(dtb)), h0=r(S, I, N), c0=r(S, K - 1, I))
    d_g = r(S, T, I)
    r64, r32 = ssm_ref(torch.float64, done, d_g=d_g, **inp), ssm_ref(torch.float32, done, d_g=d_g, **inp)
    return done, inp, d_g, r64, bars(r64, r32)


def run_conv(ctx, dev, c, done, inp, d_u=None):
    """-> u, convT (, d_u0, d_conv_w, d_conv_b) through rlx_ssm_conv_f32"""
    S, T, I, N, K = c
    f = lambda t: t.float().contiguous().to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    proj = f(torch.cat([inp["u0"], torch.zeros(S, T, I)], 2).reshape(S * T, 2 * I))
    out = dict(u=nan(S, T, I), convT=nan(S, K - 1, I))
    kw = {}
    if d_u is not None:
        out.update(d_proj=nan(S * T, 2 * I), d_conv_w=nan(K, I), d_conv_b=nan(I))
        kw = dict(d_u=f(d_u), d_proj=out["d_proj"], d_conv_w=out["d_conv_w"], d_conv_b=out["d_conv_b"])
    ctx.ssm_conv(proj, torch.from_numpy(done).to(dev), f(inp["w"]), f(inp["cb"]), out["u"], f(inp["c0"]) if K > 1 else None,
                 out["convT"] if K > 1 else None, **kw)
    out = {k: v.cpu() for k, v in out.items()}
    if d_u is not None:
        out["d_u0"] = out.pop("d_proj").reshape(S, T, 2 * I)[:, :, :I]
    return out


def run_scan(ctx, dev, c, done, inp, u, d_g=None, n_chunks=0):
    """-> g, hT (, d_u, d_dtr, d_B, d_C, d_z, d_dt_bias, d_A_log, d_D) through rlx_ssm_scan_f32"""
    S, T, I, N, K = c
    f = lambda t: t.float().contiguous().to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    xp = f(torch.cat([inp["dtr"], inp["B"], inp["C"]], 2).reshape(S * T, I + 2 * N))
    proj = f(torch.cat([torch.zeros(S, T, I), inp["z"]], 2).reshape(S * T, 2 * I))
    out = dict(g=nan(S, T, I), hT=nan(S, I, N))
    kw = {}
    if d_g is not None:
        out.update(d_u=nan(S, T, I), d_xp=nan(S, T, I + 2 * N), d_proj=nan(S, T, 2 * I), d_dt_bias=nan(I), d_A_log=nan(I, N), d_D=nan(I))
        kw = dict(d_g=f(d_g), **{k: v for k, v in out.items() if k.startswith("d_")})
    ctx.ssm_scan(f(u), xp, proj, torch.from_numpy(done).to(dev), f(inp["dtb"]), f(inp["Alog"]), f(inp["D"]), out["g"], f(inp["h0"]),
                 out["hT"], n_chunks=n_chunks, **kw)
    out = {k: v.cpu() for k, v in out.items()}
    if d_g is not None:
        dxp = out.pop("d_xp")
        out.update(d_dtr=dxp[:, :, :I], d_B=dxp[:, :, I:I + N], d_C=dxp[:, :, I + N:], d_z=out.pop("d_proj")[:, :, I:])
    return out


def check(c, got, r64, bar):
    """every tensor of got within its bar; prints error, bar and fraction per tensor"""
    for k, v in got.items():
        err = float((v.double() - r64[k]).abs().max())
        print(f"{c} {k}: max error {err:.3e}, bar {bar[k]:.3e}, fraction {err / bar[k]:.3f}")
        assert err <= bar[k], (k, err, bar[k])


@pytest.mark.parametrize("c", CASES, ids=str)
def test_conv_and_scan_match_float64(ctx, dev, c):
    done, inp, d_g, r64, bar = case(c)
    S, T = done.shape
    if c == RAGGED:       # what the case is said to contain (module docstring)
        assert done[:, 15].any() and done[:, 4].any() and (done[:, 25] & done[:, 26]).any() and done[:, T - 1].any()
        assert (done.sum(1) == 0).any() and T % 16 != 0
    assert all(float(r64[k].abs().max()) > 0 for k in r64 if k.startswith("d_"))
    conv = run_conv(ctx, dev, c, done, inp, r64["d_u"])
    if c[4] == 1:
        del conv["convT"]
    check(c, conv, r64, bar)
    check(c, run_scan(ctx, dev, c, done, inp, r64["u"], d_g), r64, bar)


@pytest.mark.parametrize("n_chunks", [1, 2, 4, 8])
def test_every_chunk_count_meets_the_same_bars(ctx, dev, n_chunks):
    done, inp, d_g, r64, bar = case(RAGGED)
    check((RAGGED, n_chunks), run_scan(ctx, dev, RAGGED, done, inp, r64["u"], d_g, n_chunks), r64, bar)


def test_two_calls_give_identical_bits(ctx, dev):
    done, inp, d_g, r64, _ = case(RAGGED)
    for a, b in ((run_conv(ctx, dev, RAGGED, done, inp, r64["d_u"]), run_conv(ctx, dev, RAGGED, done, inp, r64["d_u"])),
                 (run_scan(ctx, dev, RAGGED, done, inp, r64["u"], d_g), run_scan(ctx, dev, RAGGED, done, inp, r64["u"], d_g))):
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_two_calls_that_hand_the_carries_on_agree_with_one(ctx, dev):
    """T = 37 against 20 + 17 tokens; the caller zeroes the carries of the sequences whose token 19 ended an episode"""
    S, T, I, N, K = RAGGED
    done, inp, _, r64, bar = case(RAGGED)
    assert done[:, 19].any() and not done[:, 19].all()
    keep = torch.from_numpy(1 - done[:, 19]).float()[:, None, None]
    cut = lambda d, a, b: {k: (v[:, a:b] if v.shape[:2] == (S, T) else v) for k, v in d.items()}
    c1, c2 = (S, 20, I, N, K), (S, T - 20, I, N, K)
    conv1 = run_conv(ctx, dev, c1, done[:, :20].copy(), cut(inp, 0, 20))
    scan1 = run_scan(ctx, dev, c1, done[:, :20].copy(), cut(inp, 0, 20), r64["u"][:, :20])
    inp2 = dict(cut(inp, 20, T), c0=conv1["convT"] * keep, h0=scan1["hT"] * keep)
    conv2 = run_conv(ctx, dev, c2, done[:, 20:].copy(), inp2)
    scan2 = run_scan(ctx, dev, c2, done[:, 20:].copy(), inp2, r64["u"][:, 20:])
    check("20 + 17", dict(u=torch.cat([conv1["u"], conv2["u"]], 1), convT=conv2["convT"], g=torch.cat([scan1["g"], scan2["g"]], 1),
                          hT=scan2["hT"]), r64, bar)


@pytest.mark.parametrize("S, T, I, N, K", [(2, 5, 96, 8, 4), (2, 5, 64, 6, 4), (2, 5, 64, 8, 5), (2, 0, 64, 8, 4)], ids=["I96", "N6", "K5", "T0"])
def test_refusals_write_nothing(ctx, dev, S, T, I, N, K):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    outs = [torch.full(s, 7.0, device=dev) for s in ((S * T, I), (S, K - 1, I), (S * T, I), (S, I, N))]
    if N == 8:
        with pytest.raises(L.RlxError, match=r"rc=-4"):       # RLX_EUNSUP
            ctx.ssm_conv(z(S * T, 2 * I), z(S, T, dt=torch.uint8), z(K, I), z(I), outs[0], z(S, K - 1, I), outs[1])
    if K == 4:
        with pytest.raises(L.RlxError, match=r"rc=-4"):
            ctx.ssm_scan(z(S * T, I), z(S * T, I + 2 * N), z(S * T, 2 * I), z(S, T, dt=torch.uint8), z(I), z(I, N), z(I), outs[2], z(S, I, N),
                         outs[3])
    assert all(bool((o == 7.0).all()) for o in outs)
