"""GPU: MPO (mpo.hip) across the shape envelope rlx_mpo_desc / rlx_mpo_hparams accept, against the float64 twin
(tests/mpo_twin.py), at the bars of test_gpu_mpo.py (tests/mpo_cases.py).

Two updates per case, injected noise: step 1 from zero moments, then step 2 started from the twin's state after step 1
(teacher-forced: the bars measure the kernels, not two steps of drift).  All 11 state vectors and the 17 metrics are compared.
The paths each case is there for, worked out from the host selection code (k_mpo_sample_l1<4> for H <= 256 else <8> with
NJ = H / 64; fs_head_bwd's NJ / untiled choice; stage_dw's split-operand engine for M >= 4096 rows (bx_dw_usable); net_images
for T = 3 S B >= 4096 target rows; rows_grid's cap (mp_fwd's LayerNorm) of num_cus 8 workgroups of 4 rows, bwd_rows_grid's num_cus 4
of 16 rows, elem_grid's 4096 blocks of 256 elements -- net_pass.h); R = 2B stacked rows:

| case      | O / Op / Oc   | A  | H   | NA  | B             | S  | also                      | paths                                        |
|-----------|---------------|----|-----|-----|---------------|----|---------------------------|----------------------------------------------|
| wide      | 48 / 48 / 48  | 12 | 512 | 128 | 333           | 8  | odd B                     | sample_l1<8> NJ 8; both atom slots full;     |
|           |               |    |     |     |               |    |                           | critic head dW untiled, policy head NJ 8;    |
|           |               |    |     |     |               |    |                           | target images at H 512 (T 7992)              |
| act64     | 70 / 33 / 29  | 64 | 128 | 65  | 37            | 64 | index sets, Oc + A = 93   | every action lane and every sample lane;     |
|           |               |    |     |     |               |    |                           | second atom slot with lane 0 only;           |
|           |               |    |     |     |               |    |                           | sample_l1<4> NJ 2; k_mpo_dual at A 64;       |
|           |               |    |     |     |               |    |                           | images at H 128 (T 7104)                     |
| narrow    | 5 / 5 / 5     | 1  | 192 | 2   | 1             | 1  | v -3 .. 7, clipping on,   | NA 2 (dz = the whole range), S 1 (log S 0),  |
|           |               |    |     |     |               |    | reward past v_max         | R 2, T 3 (exact engine); sample_l1<4> NJ 3   |
| tiles     | 45 / 45 / 45  | 17 | 320 | 51  | 2053          | 2  | ragged O                  | sample_l1<8> NJ 5; critic head dW NJ 12;     |
|           |               |    |     |     |               |    |                           | R 4106 >= 4096 > B: the policy dW stays on   |
|           |               |    |     |     |               |    |                           | the exact engine, critic dW exact (B 2053)   |
| many_rows | 48 / 48 / 48  | 3  | 64  | 21  | 64 num_cus+37 | 1  | num_cus from the device   | LN forward grid cap (R > 32 num_cus) and the |
|           |               |    |     |     |               |    |                           | backward grid-stride loop (B > 64 num_cus);  |
|           |               |    |     |     |               |    |                           | k_mpo_gather grid-stride (R ldp > 2^20);     |
|           |               |    |     |     |               |    |                           | critic dW on the split engine (policy exact);|
|           |               |    |     |     |               |    |                           | k_mpo_dual sums over R ~ 33k                 |

Every B except 1 leaves the last workgroup of k_mpo_critic_loss with idle waves (B % 4 != 0), and R, T are ragged.  The profiler
confirms the engine choices it sees (k_gemm_fwd / k_gemm_dw rows, `engine` 1 = split-operand): the target critic's hidden
layers (M = T, N = K = H) on engine 1 exactly when T >= 4096; the critic's weight gradients (K = B rows) in many_rows only.  The
policy's weight gradients (K = R rows) stay on engine 0 whatever R: the actor pass keeps the exact engine because its
gradients can leave fp16's range (the mid-training cases).  With the engine switched off in the context, engine 0 everywhere.

Also: mid-training states at the default size (step 37, non-zero moments in all three optimisers, duals away from their
initial values, alpha ~ 1000, a target policy with sigma ~ 0.02-0.05 and one with sigma ~ 0.006-0.009): the twin measures the
actor's trunk gradients scaled as the split engine would scale them (bx_grad_scale) against fp16's range -- 3.8x headroom at
sigma 0.028, none at sigma 0.007, where the split engine returned a NaN gradient norm; acting at A 1 and A 64 with H 512 past
elem_grid's cap, with and without action_rescaling, sampled and deterministic; and the refusals for every field of rlx_mpo_desc /
rlx_mpo_hparams / the call arguments that were not yet tested, each before any device work."""
import re

import numpy as np
import pytest
import torch

import mpo_twin as tw
from mpo_cases import STATE_KEYS, Run, _hp, _rel, _t, check_against_twin
from rlx_amd.hip import mpo_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def bx_grad_scale(rows):
    """gemm_bx.h bx_grad_scale: 8 * 2^ceil(log2 rows)"""
    s, r = 8.0, 1
    while r < rows and s < 1e9:
        r, s = r << 1, s * 2.0
    return s


class Case:
    """a twin state (targets from their own seed), a batch with terminations, truncations and n-steps 1..4, and noise per step"""

    def __init__(self, seed, O, A, H, NA, B, S, Op=None, Oc=None, **hp):
        self.h = dict(tw.HP, action_sampling_number=S, **hp)
        rng = np.random.default_rng(seed)
        self.O, self.A, self.H, self.NA, self.B, self.S = O, A, H, NA, B, S
        self.pidx = None if Op is None else np.sort(rng.choice(O, Op, replace=False)).astype(np.int32)
        self.cidx = None if Oc is None else rng.choice(O, Oc, replace=False).astype(np.int32)
        self.Op, self.Oc = (O if Op is None else Op), (O if Oc is None else Oc)
        self.desc = mpo_desc(self.Op, self.Oc, A, H, NA)
        self.LP, self.LQ = tw.policy_layout(self.Op, A, H), tw.critic_layout(self.Oc, A, H, NA)
        p, q = tw.make_params(seed, self.Op, self.Oc, A, H, NA)
        tp, tq = tw.make_params(seed + 1000, self.Op, self.Oc, A, H, NA)
        zp, zq, nd = np.zeros(p.size), np.zeros(q.size), 2 * A + 2
        self.state = dict(p=p, pm=zp, pv=zp, tp=tp, q=q, qm=zq, qv=zq, tq=tq, d=tw.init_duals(A, self.h), dm=np.zeros(nd), dv=np.zeros(nd))
        dones = (rng.random(B) < 0.2).astype(np.float64)
        truncs = dones * (rng.random(B) < 0.5)
        nsteps = rng.integers(1, 5, B).astype(np.float64)
        nsteps[:4] = [1.0, 2.0, 3.0, 4.0][:B]
        vmax = max(abs(self.h["v_min"]), abs(self.h["v_max"]))
        rewards = _f32(rng.standard_normal(B) * min(5.0, vmax / 4))
        self.batch = [_f32(rng.standard_normal((B, O))), _f32(rng.standard_normal((B, O))), _f32(rng.standard_normal((B, A)) * 0.8),
                      rewards, dones, truncs, nsteps]
        self.rng = rng

    def noise(self):
        r = self.rng
        return _f32(r.standard_normal((self.S, self.B, self.A))), _f32(r.standard_normal((self.S, 2 * self.B, self.A)))

    def twin(self, st, eps, step):
        return tw.update(st, self.LP, self.LQ, self.batch, eps[0], eps[1], self.h, step, self.pidx, self.cidx)

    def run(self, ctx, dev, st, eps, step, key=(0, 7)):
        return Run(ctx, dev, self.desc, st, self.batch, self.h, eps, self.pidx, self.cidx, key=key, step=step)


def _shape_case(name):
    c = {
        "wide": lambda: Case(71, 48, 12, 512, 128, 333, 8),
        "act64": lambda: Case(72, 70, 64, 128, 65, 37, 64, Op=33, Oc=29),
        "narrow": lambda: Case(73, 5, 1, 192, 2, 1, 1, v_min=-3.0, v_max=7.0),
        "tiles": lambda: Case(74, 45, 17, 320, 51, 2053, 2),
        "many_rows": lambda: Case(75, 48, 3, 64, 21, 64 * _num_cus() + 37, 1),
    }[name]()
    if name == "narrow":        # the one row: not done, a reward past v_max -- every projected target sits on the top atom
        c.batch[3][:] = 8.5
        c.batch[4][:] = 0.0
        c.batch[5][:] = 0.0
    return c


NAMES = ["wide", "act64", "narrow", "tiles", "many_rows"]


def _head_nj(K, N):
    """dense_head.hip fs_head_bwd: the tiled kernel's NJ (2 / 4 / 8 / 12), 0 = the untiled kernel"""
    TK = K // 8
    TN = 256 // TK if 0 < TK <= 256 else 0
    nj = -(-N // TN) if TN else 99
    if not (K % 8 == 0 and nj <= 12 and 16 * (K + N) * 4 <= 48 * 1024):
        return 0
    return 2 if nj <= 2 else 4 if nj <= 4 else 8 if nj <= 8 else 12


@pytest.mark.parametrize("name", NAMES)
def test_shape_case_reaches_its_paths(name):
    """the case table's claims, from the host selection code's arithmetic"""
    c = _shape_case(name)
    nc = _num_cus()
    A, H, NA, B, S = c.A, c.H, c.NA, c.B, c.S
    R, T = 2 * B, 3 * S * B
    ldp = (c.Op + 3) & ~3
    sample = (4 if H <= 256 else 8, H // 64)
    heads = (_head_nj(H, 2 * A), _head_nj(H, NA))
    want = {"wide": lambda: sample == (8, 8) and NA == 128 and heads == (8, 0) and T >= 4096 > R and B % 2 == 1,
            "act64": lambda: sample == (4, 2) and A == 64 and S == 64 and NA == 65 and (c.Oc + A) % 4 != 0 and T >= 4096 and
            c.Op != c.O and c.Oc != c.O,
            "narrow": lambda: sample == (4, 3) and NA == 2 and S == 1 and R == 2 and T == 3 and A == 1 and c.h["action_clipping"] and
            c.batch[3][0] > c.h["v_max"],
            "tiles": lambda: sample == (8, 5) and heads[1] == 12 and R >= 4096 > B and R % 128 != 0 and c.O % 4 != 0,
            "many_rows": lambda: sample == (4, 1) and -(-R // 4) > 8 * nc and -(-B // 16) > 4 * nc and -(-(R * ldp) // 256) > 4096 and
            B >= 4096 and S == 1}[name]
    assert want(), (name, sample, heads)
    assert name == "many_rows" or B % 4 != 0 or B == 1


def _gemm_rows(ctx, fn):
    ctx.prof_begin()
    try:
        r = fn()
    finally:
        ctx.prof_end()
    return r, [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dw")]


def _check_engines(ctx, c, rows):
    """the engine of the target critic's hidden layers and of both weight-gradient passes, as the selection code decides it"""
    bx = ctx.get_counter("gemm_bx") == 1
    H, B, R, T = c.H, c.B, 2 * c.B, 3 * c.S * c.B
    eng = lambda pred: {q["engine"] for q in rows if pred(q)}
    if not bx:
        assert all(q["engine"] == 0 for q in rows), rows
    target = eng(lambda q: q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (T, H, H))
    assert target == {1 if bx and T >= 4096 else 0}, (target, T)
    pol = eng(lambda q: q["kernel"] == "k_gemm_dw" and q["K"] == R and q["N"] == H)
    cri = eng(lambda q: q["kernel"] == "k_gemm_dw" and q["K"] == B and q["N"] == H)
    assert pol == {0}, (pol, R)                         # the actor's weight gradients: always the exact engine
    assert cri == {1 if bx and B >= 4096 else 0}, (cri, B)


@pytest.mark.parametrize("name", NAMES)
def test_two_updates_match_the_twin(ctx, dev, name):
    c = _shape_case(name)
    eps1, eps2 = c.noise(), c.noise()
    r1, rows = _gemm_rows(ctx, lambda: c.run(ctx, dev, c.state, eps1, 1))
    st1, met1, _ = c.twin(c.state, eps1, 1)
    check_against_twin(r1, st1, met1, c.h, c.state)
    _check_engines(ctx, c, rows)
    assert np.array_equal(r1.out["d"][1:1 + c.A], c.state["d"][1:1 + c.A])           # log_alpha_mean: no gradient
    # step 2 from the twin's state (non-zero moments, moved duals), rounded to float32 for both sides
    st1 = {k: _f32(v) for k, v in st1.items()}
    r2 = c.run(ctx, dev, st1, eps2, 2, key=(3, 4))
    st2, met2, _ = c.twin(st1, eps2, 2)
    check_against_twin(r2, st2, met2, c.h, st1)


# ----------------------------------------------------------------------------------------------- mid-training at the default size
def _mid_training_case(raw=-3.2):
    """obs 48, act 12, hidden 256, 51 atoms, S 20, B 4096 at step 37: the target policy's std head pre-activation near `raw`
    (-3.2: std ~ 0.02 .. 0.05), the online policy a perturbed copy whose means sit a few KL bounds away (|mu - mu_t| ~ 0.25
    sigma_t), non-zero first and second moments in all three optimisers, duals moved from their initial values (alpha ~ 1000)"""
    c = Case(81, 48, 12, 256, 51, 4096, 20)
    sigma = 0.5 / np.log(2.0) * np.log1p(np.exp(raw))
    A, H, rng = c.A, c.H, np.random.default_rng(82)
    st = c.state
    tp = st["tp"].copy()
    o, n = c.LP["bh"]
    tp[o + A:o + 2 * A] = raw + 0.1 * rng.standard_normal(A)
    o, n = c.LP["Wh"]
    W = tp[o:o + n].reshape(H, 2 * A)
    W[:, A:] *= 0.3
    tp = _f32(tp)
    p = tp * (1.0 + 1e-3 * rng.standard_normal(tp.size))
    o, n = c.LP["bh"]
    p[o:o + A] += 0.25 * sigma * rng.standard_normal(A)
    p = _f32(p)
    q = _f32(st["tq"] * (1.0 + 0.02 * rng.standard_normal(st["tq"].size)))
    mom = lambda n, s: (_f32(s * rng.standard_normal(n)), _f32(s * s * (0.2 + rng.random(n))))
    pm, pv = mom(p.size, 3e-3)
    qm, qv = mom(q.size, 3e-4)
    d = st["d"].copy()
    d[0] = 9.2
    d[1 + A:1 + 2 * A] = 999.6 + 0.05 * rng.standard_normal(A)
    d[-1] = 9.6
    d = _f32(d)
    dm, dv = mom(2 * A + 2, 0.05)
    dm[1:1 + A] = 0.0         # log_alpha_mean never had a gradient
    dv[1:1 + A] = 0.0
    c.state = dict(st, p=p, pm=pm, pv=pv, tp=tp, q=q, qm=qm, qv=qv, d=d, dm=dm, dv=dv)
    return c


def _policy_dz_scaled(c, eps):
    """max |dZ| x bx_grad_scale(rows) of every weight-gradient operand of the actor (rows R) and critic (rows B) passes: the
    pre-activation gradients of the three trunk layers, from the twin (tensor hooks on a recording copy of its forward)"""
    seen = {}
    fwd = tw.net_fwd

    def rec(p, Lr, x):
        if not p.requires_grad:
            return fwd(p, Lr, x)
        Hh, i, o = Lr["H"], Lr["in"], Lr["out"]
        g = lambda nm, sh: tw._get(p, Lr, nm, sh)
        tag = "policy" if o == 2 * c.A else "critic"
        rows = x.shape[0]

        def hook(k):
            def f(gr):
                seen[(tag, k)] = float(gr.abs().max()) * bx_grad_scale(rows)
            return f
        z0 = x @ g("W0", (i, Hh)) + g("b0", (Hh,))
        z0.register_hook(hook(0))
        h = torch.tanh(torch.nn.functional.layer_norm(z0, (Hh,), g("g0", (Hh,)), g("be0", (Hh,)), eps=1e-5))
        z1 = h @ g("W1", (Hh, Hh)) + g("b1", (Hh,))
        z1.register_hook(hook(1))
        z2 = torch.nn.functional.elu(z1) @ g("W2", (Hh, Hh)) + g("b2", (Hh,))
        z2.register_hook(hook(2))
        return torch.nn.functional.elu(z2) @ g("Wh", (Hh, o)) + g("bh", (o,))
    tw.net_fwd = rec
    try:
        out = c.twin(c.state, eps, 37)
    finally:
        tw.net_fwd = fwd
    return out, seen


# (std head pre-activation, target std range (1st / 99th percentile), headroom of the actor's scaled trunk gradients: bounds)
MID = {"mid": (-3.2, (0.02, 0.05), (3.0, 5.0)),
       "late": (-4.6, (0.005, 0.01), (0.5, 1.0))}


@pytest.mark.parametrize("name", ["mid", "late"])
def test_mid_training_state_at_the_default_size(ctx, dev, name):
    """the whole update at step 37 against the twin.  The actor's per-sample trunk gradients, scaled as the split engine scales
    its gradient operands, pass fp16's range in `late`: that pass must stay on the exact engine (it returned NaN on the split
    one).  The critic's pass (B 4096 rows) keeps the split engine."""
    raw, (lo, hi), (h_lo, h_hi) = MID[name]
    c = _mid_training_case(raw)
    eps = c.noise()
    r, rows = _gemm_rows(ctx, lambda: c.run(ctx, dev, c.state, eps, 37))
    (new, met, ex), scaled = _policy_dz_scaled(c, eps)
    # the state is the one the docstring promises
    mt, sdt = tw.policy_get_action(tw._t(c.state["tp"]), c.LP, tw._t(np.concatenate([c.batch[0], c.batch[1]])), c.h)
    sd = np.percentile(sdt.numpy(), [1, 99])
    assert lo < sd[0] and sd[1] < hi, sd
    assert 999.0 < met[8] < 1001.0 and 2 * c.h["epsilon_parametric_mu"] < met[10] < 10 * c.h["epsilon_parametric_mu"], met
    headroom = F16_MAX / max(v for k, v in scaled.items() if k[0] == "policy")
    assert len(scaled) == 6 and h_lo < headroom < h_hi, scaled
    assert F16_MAX / max(v for k, v in scaled.items() if k[0] == "critic") > 1e3, scaled
    finite = [k for k in STATE_KEYS if np.all(np.isfinite(r.out[k]))]
    assert torch.isfinite(r.met).all() and len(finite) == len(STATE_KEYS), (r.metrics, finite)
    check_against_twin(r, new, met, c.h, c.state)
    if ctx.get_counter("gemm_bx") == 1:
        assert any(q["engine"] == 1 and q["kernel"] == "k_gemm_dw" and q["K"] == c.B for q in rows)
    _check_engines(ctx, c, rows)


# ----------------------------------------------------------------------------------------------------------------------- acting
def _act_cases():
    return {"a1": dict(seed=91, N=300, O=7, A=1, H=64, Op=None),
            "a64": dict(seed=92, N=16385, O=40, A=64, H=512, Op=29)}       # N A > elem_grid's 4096 x 256: grid-stride


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("name", ["a1", "a64"])
def test_act_matches_the_twin(ctx, dev, name, rescale):
    kw = _act_cases()[name]
    N, O, A, H = kw["N"], kw["O"], kw["A"], kw["H"]
    rng = np.random.default_rng(kw["seed"])
    pidx = None if kw["Op"] is None else np.sort(rng.choice(O, kw["Op"], replace=False)).astype(np.int32)
    Op = O if pidx is None else len(pidx)
    desc = mpo_desc(Op, O, A, H, 21)
    p, _ = tw.make_params(kw["seed"], Op, O, A, H, 21)
    h = dict(tw.HP, policy_init_scale=1.5, action_rescaling=rescale)          # samples leave [-1, 1]: the clamp acts
    LP = tw.policy_layout(Op, A, H)
    obs = _f32(rng.standard_normal((N, O)))
    eps = _f32(rng.standard_normal((N, A)))
    low = _f32(-1.0 - rng.random(A))
    high = _f32(low + 0.5 + 2.0 * rng.random(A))
    P, x = _t(p, dev), _t(obs, dev)
    pi = None if pidx is None else _t(pidx, dev, np.int32)
    act, proc = torch.empty(N, A, device=dev), torch.empty(N, A, device=dev)
    lo, hi = (_t(low, dev), _t(high, dev)) if rescale else (None, None)
    te = _t(eps, dev)
    key = L.prng_key(4)
    ctx.dbg_set_sac_noise(te, None)
    try:
        k1 = ctx.mpo_act(desc, P, x, key, act, proc, _hp(h), lo, hi, pidx=pi)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    assert np.array_equal(k1, key)                     # injected noise: the key is not split
    xo = obs if pidx is None else obs[:, pidx]
    ra, rp = tw.act(p, LP, xo, eps, h, low, high)
    assert np.abs(ra).max() > 1.0
    assert _rel(act.cpu().numpy(), ra) < 1e-5 and _rel(proc.cpu().numpy(), rp) < 1e-5
    if not rescale:
        assert np.abs(proc.cpu().numpy()).max() <= 1.0
    ctx.mpo_act(desc, P, x, key, act, proc, _hp(h), lo, hi, deterministic=True, pidx=pi)
    da, dp = tw.act(p, LP, xo, None, h, low, high, deterministic=True)
    assert _rel(act.cpu().numpy(), da) < 1e-5 and _rel(proc.cpu().numpy(), dp) < 1e-5


# --------------------------------------------------------------------------------------------------------------------- refusals
EINVAL, EUNSUP = -1, -4
SENTINEL = 1234.5


def _refusals():
    """(name, desc overrides, hparam overrides, call overrides, code, message fragment, entry points)"""
    both, upd, act = ("update", "act"), ("update",), ("act",)
    return [
        ("v_equal", {}, dict(v_min=5.0, v_max=5.0), {}, EINVAL, "v_max > v_min", both),
        ("v_below", {}, dict(v_min=5.0, v_max=-5.0), {}, EINVAL, "v_max > v_min", both),
        ("hidden0", dict(hidden=0), {}, {}, EINVAL, "positive widths", both),
        ("hidden-64", dict(hidden=-64), {}, {}, EINVAL, "positive widths", both),
        ("atoms0", dict(nr_atoms=0), {}, {}, EINVAL, "positive widths", both),
        ("policy_width_no_pidx", dict(policy_obs_dim=6), {}, dict(pidx=None), EINVAL, "needs", both),
        ("critic_width_no_cidx", dict(critic_obs_dim=6), {}, dict(cidx=None), EINVAL, "needs", upd),
        ("step0", {}, {}, dict(step=0), EINVAL, "bad args", upd),
        ("rows0", {}, {}, dict(rows=0), EINVAL, "bad args", both),
        ("rescale_no_bounds", {}, dict(action_rescaling=True), dict(low=None), EINVAL, "needs low and high", act),
    ]


REFUSALS = [(e, r) for r in _refusals() for e in r[6]]


@pytest.mark.parametrize("entry,r", REFUSALS, ids=["%s-%s" % (e, r[0]) for e, r in REFUSALS])
def test_envelope_refusals(ctx, dev, entry, r):
    """a value just outside each limit: the documented code (RlxError), rlx_last_error() names it, and nothing is written
    (outputs prefilled with a sentinel; parameters, moments, duals and the key unchanged); the context then runs a valid call"""
    name, dover, hover, kover, code, msg, _ = r
    O, A, H, NA, B, S = 8, 3, 64, 21, 12, 4
    c = Case(95, O, A, H, NA, B, S)
    dd = dict(dict(policy_obs_dim=O, critic_obs_dim=O, act_dim=A, hidden=H, nr_atoms=NA), **dover)
    desc = mpo_desc(*(dd[k] for k in ("policy_obs_dim", "critic_obs_dim", "act_dim", "hidden", "nr_atoms")))
    h = dict(c.h, **hover)
    rows = kover.get("rows", B)
    key = L.prng_key(3)
    key0 = key.copy()
    fill = lambda *sh: torch.full(sh, SENTINEL, device=dev)
    pi = None if kover.get("pidx", 1) is None else _t(np.arange(dd["policy_obs_dim"]), dev, np.int32)
    ci = None if kover.get("cidx", 1) is None else _t(np.arange(dd["critic_obs_dim"]), dev, np.int32)
    if entry == "act":
        P = _t(c.state["p"], dev)
        P0 = P.clone()
        obs = _t(c.batch[0][:rows], dev)
        a, pa = fill(max(rows, 1), A), fill(max(rows, 1), A)
        lo = None if "low" in kover else _t(-np.ones(A), dev)
        hi = None if "low" in kover else _t(np.ones(A), dev)
        with pytest.raises(L.RlxError) as e:
            ctx.mpo_act(desc, P, obs, key, a, pa, _hp(h), lo, hi, pidx=pi)
        outs, same = [a, pa], [(P, P0)]
    else:
        nets = tuple(_t(c.state[k], dev) for k in STATE_KEYS)
        for t in nets[1:3] + nets[5:7] + nets[9:]:
            t.fill_(SENTINEL)
        before = [x.clone() for x in nets]
        met = fill(17)
        batch = tuple(_t(x[:rows], dev) for x in c.batch)
        with pytest.raises(L.RlxError) as e:
            ctx.mpo_update(desc, nets, batch, key, kover.get("step", 1), 3e-4, 1e-2, _hp(h), met, pidx=pi, cidx=ci)
        outs, same = [met], list(zip(nets, before))
    text = str(e.value)
    rc = int(re.search(r"rc=(-?\d+)", text).group(1))
    assert rc == code and msg in text, text
    assert msg in L.load_library().rlx_last_error().decode()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), name
    for x, y in same:
        assert torch.equal(x, y), name
    assert np.array_equal(key, key0)
    # the context still serves a valid call
    good = Case(96, O, A, H, NA, B, S)
    g = good.run(ctx, dev, good.state, good.noise(), 1)
    assert np.all(np.isfinite(g.metrics)) and g.metrics[0] > 0


def test_param_count_refuses_bad_descriptors(ctx):
    import ctypes
    lib = L.load_library()
    count = lambda d, net: lib.rlx_mpo_param_count(ctypes.byref(d), net)
    good = mpo_desc(8, 8, 3, 64, 21)
    assert count(good, 0) == tw.policy_layout(8, 3, 64)["n"] and count(good, 1) == tw.critic_layout(8, 3, 64, 21)["n"]
    assert count(good, 2) == 2 * 3 + 2
    assert count(good, 3) == -1 and count(good, -1) == -1
    for d in (mpo_desc(8, 8, 0, 64, 21), mpo_desc(8, 8, -2, 64, 21), mpo_desc(8, 8, 3, 0, 21), mpo_desc(8, 8, 3, -64, 21)):
        for net in (0, 1, 2):
            assert count(d, net) == -1, (d.act_dim, d.hidden, net)
    assert lib.rlx_mpo_param_count(None, 0) == -1
