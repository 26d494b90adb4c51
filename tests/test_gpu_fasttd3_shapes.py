"""GPU: FastTD3 (fasttd3.hip) across the shape envelope td3_check / td3_check_pair accept, against the float64 twin
(tests/fasttd3_twin.py), at the bars of test_gpu_fasttd3.py (tests/fasttd3_cases.py states them, with the ReLU-kink / tie accounting
those tests use: candidates counted from float64 alone, at most MAX_FLIPS explained per update step; test_fasttd3_cases.py holds
a float32 evaluation on the CPU to the same condition).

Two steps per case, injected smoothing noise: step 1 (a critic update and a policy update) from zero moments, then step 2
started from the twin's state after step 1, rounded to float32 for both sides (teacher-forced; opt_count 1).  All seven state
vectors (P, pm, pv, Q, qm, qv, QT) and all six metrics are compared.  The paths each case is there for, recomputed in
test_shape_case_reaches_its_paths from a mirror of the host selection code (tests/net_paths.py; num_cus from the device):

| case         | O / Op / Oc  | A  | policy hidden  | critic hidden  | NA  | B               | paths                                          |
|--------------|--------------|----|----------------|----------------|-----|-----------------|------------------------------------------------|
| narrow       | 5 / 5 / 5    | 1  | (64)           | (64)           | 2   | 1               | one layer, one row, A 1, NA 2 with a reward    |
|              |              |    |                |                |     |                 | past v_max; dx_cols with one column; clipped   |
| wide         | 48 / 48 / 48 | 16 | (1024, 64)     | (1024, 1024)   | 128 | 333             | width 1024; critic head K 1024 untiled, fused  |
|              |              |    |                |                |     |                 | policy head at K 64; dx_cols' LDS bound fails  |
|              |              |    |                |                |     |                 | at A 16: whole-GEMM first_layer_dx; mean of two|
| act64        | 70 / 33 / 29 | 64 | (128, 64, 64)  | (128, 64, 64)  | 65  | 37              | critic_states and critic_next_states; Oc + A = |
|              |              |    |                |                |     |                 | 93 ragged; dx_cols with 64 columns at an       |
|              |              |    |                |                |     |                 | unaligned base; max_grad_norm active; clipped  |
| split3       | 48 / 48 / 48 | 12 | (256, 128, 64) | (256, 128, 64) | 51  | 4099            | 15 matrices / 19 image jobs: every trunk GEMM  |
|              |              |    |                |                |     |                 | on the split engine; B % 4 != 0; mean of two   |
| split_ragged | 45 / 45 / 45 | 17 | (256, 128, 64) | (256, 128, 64) | 101 | 4099            | ragged first layers (45, 62) stay exact, their |
|              |              |    |                |                |     |                 | weight gradients and the later layers split;   |
|              |              |    |                |                |     |                 | clipped                                        |
| many_rows    | 64 / 64 / 64 | 64 | (64)           | (64)           | 21  | 64 num_cus + 37 | elem_grid's cap in k_td3_head_act and          |
|              |              |    |                |                |     |                 | k_td3_tanh_bwd (B A > 2^20), fs_concat's cap,  |
|              |              |    |                |                |     |                 | > 256 loss partials; mean of two               |
| head320      | 1 / 1 / 1    | 1  | (64, 320)      | (64, 320)      | 21  | 13              | the heads' input gradient with its ReLU'       |
|              |              |    |                |                |     |                 | epilogue (8 rows per workgroup, the width in   |
|              |              |    |                |                |     |                 | strides of 256): a last workgroup of 5 rows, a |
|              |              |    |                |                |     |                 | second stride with 64 threads active; clipped  |

The profiler confirms the engine of every trunk GEMM it sees (net_paths.expected_engines), and everything runs on engine 0 with the
split engine switched off in the context.  Also: acting at A 1 and at A 64 with N A past elem_grid's cap, against the twin and over
a row range of a global batch; the two-stream schedule bit for bit at the ragged act64 shape; and a refusal per limit of td3_check /
td3_check_pair / the entry points' argument checks, each before any device work.

Measured on the MI355X (split-operand engine on), ||dg|| / ||g|| of the first step's (critic, policy) gradient after the flips taken
(in brackets; candidates inside KINK_TAU): narrow 4.1e-7, 3.4e-7 (0 of 0, 0 of 0); wide 1.3e-6, 3.2e-7 (0 of 2, 0 of 3); act64
1.1e-6, 3.0e-7 (0 of 0, 0 of 0); split3 2.4e-7, 2.2e-7 (0 of 9, 1 of 20: 3.6e-5 before, the unit-sample the CPU float32 evaluation
flips too); split_ragged 2.9e-7, 2.4e-7 (1 of 7: 5.7e-5 before; 0 of 13); many_rows 2.4e-7, 2.2e-7 (0 of 4, 0 of 9).  The second
step lands at 9e-8 .. 1.9e-6 ("Shape envelope of FastSAC and FastTD3")."""
import ctypes
import re

import numpy as np
import pytest
import torch

import fasttd3_cases as fc
import fasttd3_twin as tw
import net_paths as npth
from fasttd3_cases import _f32, _hp, _rel, _t
from rlx_amd.hip import lib as L
from rlx_amd.hip import relu_mlp_desc

pytestmark = pytest.mark.gpu
NAMES = fc.NAMES


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(name):
    return fc.shape_case(name, _num_cus())


@pytest.mark.parametrize("name", NAMES)
def test_shape_case_reaches_its_paths(name):
    """the case table's claims, from the host selection code's arithmetic"""
    c = _case(name)
    A, NA, B, Op, Oc = c.A, c.NA, c.B, c.Op, c.Oc
    ldc, ldp = npth.pad4(Oc + A), npth.pad4(Op)
    heads = (npth.head_nj(c.ph[-1], A), npth.head_nj(c.ch[-1], NA))
    dxc = npth.dx_cols_ok(c.ch[0], A)
    cu = npth.trunk_images([(Op, c.ph, False)] + [(Oc + A, c.ch, False)] * 2 + [(Oc + A, c.ch, True)] * 2)
    pu = npth.trunk_images([(Op, c.ph, True)] + [(Oc + A, c.ch, True)] * 2)
    want = {
        "narrow": lambda: len(c.ph) == len(c.ch) == 1 and B == 1 and A == 1 and NA == 2 and dxc and c.batch[3][0] > c.h["v_max"] and c.clipped,
        "wide": lambda: max(c.ph + c.ch) == 1024 and c.ch[-1] == 1024 and heads == (2, 0) and not dxc and npth.dx_cols_ok(c.ch[0], A - 1) and
        NA == 128 and B % 2 == 1 and B < 4096 and not c.clipped,
        "act64": lambda: c.split and Op != Oc and (Oc + A) % 4 != 0 and A == 64 and dxc and Oc % 4 != 0 and len(c.ch) == 3 and NA == 65 and
        B < 4096 and c.h["max_grad_norm"] > 0,
        "split3": lambda: B >= 4096 and B % 4 != 0 and cu[:2] == (15, 19) and pu[:2] == (9, 15) and Op % 4 == 0 and (Oc + A) % 4 == 0 and dxc,
        "split_ragged": lambda: B >= 4096 and Op % 4 != 0 and (Oc + A) % 4 != 0 and cu[:2] == (10, 14) and pu[:2] == (6, 12) and dxc and
        npth.bx_dw_usable(True, B, Oc + A, ldc, c.ch[0]) and npth.bx_dw_usable(True, B, Op, ldp, c.ph[0]) and c.clipped,
        "many_rows": lambda: npth.elem_grid(B * A)[1] and npth.elem_grid(B * ldc)[1] and npth.div_up(B, 4) > 256 and B >= 4096 and dxc and A == 64,
        "head320": lambda: c.ph[-1] == c.ch[-1] == 320 and 256 < 320 < 512 and B > 8 and B % 8 == 5 and Op == Oc == A == 1 and c.clipped,
    }[name]
    assert want(), (name, heads, dxc, cu[:2], pu[:2])
    assert name == "many_rows" or B % 4 != 0 or B == 1
    assert cu[1] <= npth.BX_MAX_JOBS and pu[1] <= npth.BX_MAX_JOBS


def _check_engines(ctx, c, r):
    bx = ctx.get_counter("gemm_bx") == 1
    for k, update in enumerate(("critic", "policy")):
        exp = npth.expected_engines(update, bx, c.B, c.Op, c.ph, c.Oc + c.A, c.ch, c.A)
        if not bx or c.B < npth.SPLIT_ROWS:
            assert set(exp.values()) == {0}
        npth.check_engines(r.prof[k], exp)


@pytest.mark.parametrize("name", NAMES)
def test_two_updates_match_the_twin(ctx, dev, name):
    c = _case(name)
    eps1, eps2 = c.noise(), c.noise()
    r1 = c.run(ctx, dev, c.state, eps1, 1, profile=True)
    res, st1 = fc.check_against_twin(c, r1, c.state, eps1, 1, name)
    _check_engines(ctx, c, r1)
    if c.B >= npth.SPLIT_ROWS:          # what the split engine's operands reach, from the twin (headroom > 50x, 50x, 10x)
        w = fc.fp16_window(c, c.state, eps1)
        print(f"FastTD3 {name}: max |w| {w['weight']:.3g} (< 1023), max |act| {w['act']:.3g} (< 4094), scaled gradient {w['grad_scaled']:.3g} (< 65504)")
        assert w["weight"] * 50 < npth.X_WLIMIT and w["act"] * 50 < npth.X_ALIMIT and 0 < w["grad_scaled"] * 10 < npth.F16_MAX, w
    if c.h["max_grad_norm"] > 0:
        assert r1.cmetrics[3] > c.h["max_grad_norm"] and r1.pmetrics[1] > c.h["max_grad_norm"]
    # step 2 from the twin's state (non-zero moments, bias correction at step 2), rounded to float32 for both sides
    st1 = {k: _f32(v) for k, v in st1.items()}
    r2 = c.run(ctx, dev, st1, eps2, 2, key=(3, 4))
    fc.check_against_twin(c, r2, st1, eps2, 2, name)


def test_split_engine_off_runs_the_exact_engine(ctx, dev):
    """counter gemm_bx = 0: everything on engine 0 at 4099 rows too, same bars"""
    c = _case("split3")
    eps = c.noise()
    ctx.set_option("gemm_bx", 0)
    try:
        assert ctx.get_counter("gemm_bx") == 0
        r = c.run(ctx, dev, c.state, eps, 1, profile=True)
        _check_engines(ctx, c, r)
    finally:
        ctx.set_option("gemm_bx", 1)
    fc.check_against_twin(c, r, c.state, eps, 1, "split3, exact engine")


# ----------------------------------------------------------------------------------------------------------------------- acting
ACT = {"a1": (281, 300, 7, 1, (64,)), "a64": (282, 16400, 40, 64, (64,))}      # a64: N A > elem_grid's 4096 x 256: grid-stride


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", list(ACT))
def test_act_matches_the_twin(ctx, dev, name, clip):
    seed, N, O, A, hidden = ACT[name]
    rng = np.random.default_rng(seed)
    assert npth.elem_grid(N * A)[1] == (name == "a64")
    p, _ = tw.make_params(seed, O, A, 21, policy_hidden=hidden, critic_hidden=(64,))
    pd = relu_mlp_desc(O, hidden, A)
    obs, eps = _f32(rng.standard_normal((N, O))), _f32(2.0 * rng.standard_normal((N, A)))
    scales = _f32(rng.uniform(0.1, 0.9, N))
    low, high = (_f32(-1.0 - rng.random(A)), _f32(0.5 + rng.random(A))) if clip else (None, None)
    P, x = _t(p, dev), _t(obs, dev)
    act, proc = torch.full((N, A), 1234.5, device=dev), torch.full((N, A), 1234.5, device=dev)
    lo, hi = (_t(low, dev), _t(high, dev)) if clip else (None, None)
    key = L.prng_key(4)
    te = _t(eps, dev)
    ctx.dbg_set_sac_noise(te, None)
    try:
        ctx.fasttd3_act(pd, P, x, _t(scales, dev), key, act, proc, low=lo, high=hi)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    ea, ep = tw.act(p, O, A, obs, eps, scales, low, high, hidden)
    assert _rel(act.cpu().numpy(), ea) < 1e-5 and _rel(proc.cpu().numpy(), ep) < 1e-5
    assert np.abs(ea).max() > 1.0                       # the clamp of clip-and-rescale acts
    k1 = ctx.fasttd3_act(pd, P, x, None, key, act, proc, deterministic=True, low=lo, high=hi)
    assert np.array_equal(k1, key)                      # nothing drawn: the key is untouched
    da, dp = tw.act(p, O, A, obs, None, None, low, high, hidden)
    assert _rel(act.cpu().numpy(), da) < 1e-5 and _rel(proc.cpu().numpy(), dp) < 1e-5


def test_act_on_a_row_range_equals_the_rows_of_the_full_call(ctx, dev):
    """the library's own draws: rows [r0, r0 + N) with row_offset = r0, n_global = NG are bit for bit the rows of the NG-row call"""
    seed, NG, O, A, hidden = 285, 301, 9, 3, (64,)
    rng = np.random.default_rng(seed)
    p, _ = tw.make_params(seed, O, A, 21, policy_hidden=hidden, critic_hidden=(64,))
    pd = relu_mlp_desc(O, hidden, A)
    P, x, sc = _t(p, dev), _t(rng.standard_normal((NG, O)), dev), _t(rng.uniform(0.1, 0.9, NG), dev)
    full, fproc = torch.empty(NG, A, device=dev), torch.empty(NG, A, device=dev)
    key = L.prng_key(9)
    k_full = ctx.fasttd3_act(pd, P, x, sc, key, full, fproc)
    assert not np.array_equal(k_full, key) and full.std().item() > 0.05
    for r0, n in ((0, 86), (86, 170), (256, 45)):
        part, pproc = torch.empty(n, A, device=dev), torch.empty(n, A, device=dev)
        k = ctx.fasttd3_act(pd, P, x[r0:r0 + n].contiguous(), sc[r0:r0 + n].contiguous(), key, part, pproc, row_offset=r0, n_global=NG)
        assert np.array_equal(k, k_full) and torch.equal(part, full[r0:r0 + n]) and torch.equal(pproc, fproc[r0:r0 + n]), r0


# ---------------------------------------------------------------------------------------------------------- two-stream schedule
def test_two_stream_schedule_is_bit_identical_at_a_ragged_shape(ctx, dev):
    """two_streams 0 against 1 at act64: critic_states, ragged Oc + A, dx_cols at an unaligned base"""
    c = _case("act64")
    eps = c.noise()

    def run(two):
        ctx.set_option("two_streams", two)
        r = c.run(ctx, dev, c.state, eps, 1)
        return [r.out[k] for k in fc.STATE_KEYS] + [r.cmetrics, r.pmetrics]
    try:
        one, two = run(0), run(1)
    finally:
        ctx.set_option("two_streams", 1)
    for x, y, k in zip(one, two, fc.STATE_KEYS + ("critic metrics", "policy metrics")):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y), k


# --------------------------------------------------------------------------------------------------------------------- refusals
EINVAL, EUNSUP = -1, -4
SENTINEL = 1234.5
GOOD = dict(O=8, A=3, ph=(64, 64), ch=(64, 64), NA=21, B=12)


def _refusals():
    """(name, overrides, code, message fragment, entry points).  Overrides: pd / qd = (in_dim, hidden, out_dim[, act, ln_first,
    has_logstd]) of the policy / critic descriptor, hparams by name, cs / cn = pass critic_states / critic_next_states, rows,
    n_global, no_scales (sampled acting without noise scales), clip_no_bounds"""
    O, A, NA = GOOD["O"], GOOD["A"], GOOD["NA"]
    all3, upd, act = ("critic", "policy", "act"), ("critic", "policy"), ("act",)
    pd = lambda hidden, out=A, *flags: dict(pd=(O, hidden, out) + flags)
    qd = lambda hidden, i=O + A, out=NA, *flags: dict(qd=(i, hidden, out) + flags)
    lmsg, wmsg, dmsg = "1..3 hidden layers", "multiples of 64, at most 1024", "act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0"
    return [
        ("policy_0_layers", pd(()), EINVAL, lmsg, all3),
        ("policy_4_layers", pd((64,) * 4), EINVAL, lmsg, all3),
        ("critic_0_layers", qd(()), EINVAL, lmsg, upd),
        ("critic_4_layers", qd((64,) * 4), EINVAL, lmsg, upd),
        ("policy_width_0", pd((64, 0)), EUNSUP, wmsg, all3),
        ("policy_width_96", pd((96, 64)), EUNSUP, wmsg, all3),
        ("policy_width_1088", pd((1088,)), EUNSUP, wmsg, all3),
        ("critic_width_0", qd((0,)), EUNSUP, wmsg, upd),
        ("critic_width_96", qd((64, 96)), EUNSUP, wmsg, upd),
        ("critic_width_1088", qd((1088, 64)), EUNSUP, wmsg, upd),
        ("policy_out_0", pd((64, 64), 0), EINVAL, "positive widths", all3),
        ("policy_tanh", pd((64, 64), A, L.ACT_TANH, 0, 0), EINVAL, dmsg, all3),
        ("policy_ln_first", pd((64, 64), A, L.ACT_RELU, 1, 0), EINVAL, dmsg, all3),
        ("policy_has_logstd", pd((64, 64), A, L.ACT_RELU, 0, 1), EINVAL, dmsg, all3),
        ("critic_elu", qd((64, 64), O + A, NA, L.ACT_ELU, 0, 0), EINVAL, dmsg, upd),
        ("critic_ln_first", qd((64, 64), O + A, NA, L.ACT_RELU, 1, 0), EINVAL, dmsg, upd),
        ("act_dim_65", dict(pd=(O, (64, 64), 65), qd=(O + 65, (64, 64), NA)), EUNSUP, "at most 64", all3),
        ("critic_in_is_act", qd((64, 64), A), EINVAL, "critic in_dim = critic obs + act", upd),
        ("critic_out_not_atoms", qd((64, 64), O + A, NA + 1), EINVAL, "out_dim = nr_atoms", upd),
        ("atoms_1", dict(qd=(O + A, (64, 64), 1), nr_atoms=1), EINVAL, "nr_atoms (2..128)", upd),
        ("atoms_129", dict(qd=(O + A, (64, 64), 129), nr_atoms=129), EINVAL, "nr_atoms (2..128)", upd),
        ("v_equal", dict(v_min=5.0, v_max=5.0), EINVAL, "v_max > v_min", upd),
        ("v_below", dict(v_min=5.0, v_max=-5.0), EINVAL, "v_max > v_min", upd),
        ("critic_width_without_critic_states", qd((64, 64), O + A + 2), EINVAL, "needs critic_states", upd),
        ("only_critic_states", dict(cs=True), EINVAL, "critic_states AND critic_next_states", ("critic",)),
        ("only_critic_next_states", dict(cn=True), EINVAL, "critic_states AND critic_next_states", ("critic",)),
        ("rows_0", dict(rows=0), EINVAL, "bad args", all3),
        ("n_global_below_n", dict(n_global=GOOD["B"] - 1), EINVAL, "bad args", act),
        ("sampled_without_noise_scales", dict(no_scales=True), EINVAL, "bad args", act),
        ("clip_and_rescale_without_bounds", dict(clip_no_bounds=True), EINVAL, "bad args", act),
    ]


REFUSALS = [(e, r) for r in _refusals() for e in r[4]]


def _desc(t):
    return relu_mlp_desc(*t) if len(t) == 3 else L.mlp_desc(*t)


@pytest.mark.parametrize("entry,r", REFUSALS, ids=["%s-%s" % (e, r[0]) for e, r in REFUSALS])
def test_envelope_refusals(ctx, dev, entry, r):
    """a value just outside each limit: the documented code (RlxError), rlx_last_error() names it, and nothing is written (outputs
    prefilled with a sentinel; parameters, moments, the key and the count unchanged); the context then runs a valid call"""
    name, over, code, msg, _ = r
    O, A, NA, B = GOOD["O"], GOOD["A"], GOOD["NA"], GOOD["B"]
    c = fc.Case(295, O, A, GOOD["ph"], GOOD["ch"], NA, B)
    pd = _desc(over["pd"]) if "pd" in over else c.pd
    qd = _desc(over["qd"]) if "qd" in over else c.qd
    h = dict(c.h, **{k: v for k, v in over.items() if k in c.h})
    hp = _hp(h, over.get("nr_atoms", NA), True)
    rows = over.get("rows", B)
    key = L.prng_key(3)
    fill = lambda *sh: torch.full(sh, SENTINEL, device=dev)
    st = {k: _t(c.state[k], dev) for k in fc.STATE_KEYS}
    for k in ("pm", "pv", "qm", "qv"):
        st[k].fill_(SENTINEL)
    before = {k: v.clone() for k, v in st.items()}
    batch = tuple(_t(x, dev) for x in c.batch)          # valid buffers whatever `rows` says: the row count alone decides
    extra = fill(B, O + 2)
    lib = L.load_library()
    cnt = ctypes.c_int64(5)
    karr = (ctypes.c_uint32 * 2)(int(key[0]), int(key[1]))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    if entry == "act":
        outs = [fill(B, 65), fill(B, 65)]
        sc_t = fill(B)
        scales = None if over.get("no_scales") else ptr(sc_t)
        rc = lib.rlx_fasttd3_act_f32(ctx.h, ctypes.byref(pd), ptr(st["P"]), ptr(batch[0]), scales, karr, L.THREEFRY_PARTITIONABLE, ptr(outs[0]),
                                     ptr(outs[1]), rows, 0, 1 if over.get("clip_no_bounds") else 0, None, None, 0, over.get("n_global", rows),
                                     None)
    elif entry == "critic":
        outs = [fill(4)]
        cs = ptr(extra) if over.get("cs") else None
        cn = ptr(extra) if over.get("cn") else None
        rc = lib.rlx_fasttd3_critic_update_f32(
            ctx.h, ctypes.byref(pd), ptr(st["P"]), ctypes.byref(qd), ptr(st["Q"]), ptr(st["qm"]), ptr(st["qv"]), ptr(st["QT"]), ptr(batch[0]),
            ptr(batch[1]), cs, cn, *[ptr(x) for x in batch[2:]], rows, karr, L.THREEFRY_PARTITIONABLE, ctypes.byref(cnt), ctypes.byref(hp),
            ptr(outs[0]), None)
    else:
        outs = [fill(2)]
        rc = lib.rlx_fasttd3_policy_update_f32(
            ctx.h, ctypes.byref(pd), ptr(st["P"]), ptr(st["pm"]), ptr(st["pv"]), ctypes.byref(qd), ptr(st["Q"]), ptr(batch[0]), None, rows,
            ctypes.byref(cnt), ctypes.byref(hp), ptr(outs[0]), None)
    assert rc == code, (name, rc)
    assert msg in lib.rlx_last_error().decode(), lib.rlx_last_error().decode()
    with pytest.raises(L.RlxError) as e:                 # the binding raises the same code and message
        L._check(rc, "rlx_fasttd3")
    assert int(re.search(r"rc=(-?\d+)", str(e.value)).group(1)) == code and msg in str(e.value)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), name
    for k in fc.STATE_KEYS:
        assert torch.equal(st[k], before[k]), (name, k)
    assert (karr[0], karr[1]) == (int(key[0]), int(key[1])) and cnt.value == 5
    # the context still serves a valid call
    good = fc.Case(296, O, A, GOOD["ph"], GOOD["ch"], NA, B)
    g = good.run(ctx, dev, good.state, good.noise(), 1)
    assert np.all(np.isfinite(g.cmetrics)) and np.all(np.isfinite(g.pmetrics)) and g.cmetrics[0] > 0
