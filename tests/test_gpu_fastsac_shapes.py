"""GPU: FastSAC (fastsac.hip) across the shape envelope ln_check / fs_check accept, against the float64 oracle (oracle/fastsac.py),
at the bars of test_gpu_fastsac.py (tests/fastsac_cases.py states them).

Two steps per case, injected noise: step 1 (a critic update and a policy update) from zero moments, then step 2 started from
the oracle's state after step 1, rounded to float32 for both sides (teacher-forced: the bars measure the kernels, not two steps of
drift; opt_count 1).  All ten state vectors (P, pm, pv, Q, qm, qv, QT, log_alpha, am, av) and all eleven metrics are compared.
The paths each case is there for, recomputed in test_shape_case_reaches_its_paths from a mirror of the host selection code
(tests/net_paths.py; num_cus from the device):

| case         | O / Op / Oc  | A  | policy hidden      | critic hidden      | NA  | B              | paths                                     |
|--------------|--------------|----|--------------------|--------------------|-----|----------------|-------------------------------------------|
| narrow       | 5 / 5 / 5    | 1  | (64)               | (64)               | 2   | 1              | one layer, one row, A 1 (k_fs_sample: 256 |
|              |              |    |                    |                    |     |                | rows a block), NA 2 (dz = the range) with |
|              |              |    |                    |                    |     |                | a reward past v_max, both heads NJ 2,     |
|              |              |    |                    |                    |     |                | dx_cols with one column, clipped double Q |
| wide         | 48 / 48 / 48 | 12 | (768, 704)         | (768, 768)         | 128 | 333            | LayerNorm width 768; policy head K 704:   |
|              |              |    |                    |                    |     |                | NJ 12 with 80 masked threads; critic head |
|              |              |    |                    |                    |     |                | K 768 untiled (16 (K + N) floats > 48 KB);|
|              |              |    |                    |                    |     |                | both atom slots full; odd B               |
| act65        | 70 / 33 / 29 | 65 | (128, 64, 64, 64)  | (128, 64, 64, 64)  | 65  | 37             | critic_states and critic_next_states;     |
|              |              |    |                    |                    |     |                | Oc + A = 94 ragged; A > 64: first_layer_dx|
|              |              |    |                    |                    |     |                | through the whole GEMM; four layers on the|
|              |              |    |                    |                    |     |                | exact engine; second atom slot with lane 0|
|              |              |    |                    |                    |     |                | only; max_grad_norm active; clipped       |
| dxlds        | 45 / 45 / 45 | 27 | (256, 128)         | (768, 192)         | 51  | 130            | A <= 64 but dx_cols' LDS bound fails at   |
|              |              |    |                    |                    |     |                | width 768 (whole GEMM, Kd 72); Oc % 4 != 0|
|              |              |    |                    |                    |     |                | ; policy head NJ 4, critic head NJ 8 (the |
|              |              |    |                    |                    |     |                | defaults reach NJ 2 and NJ 12 only)       |
| split4       | 48 / 48 / 48 | 4  | (128, 64, 64, 64)  | (128, 64, 64, 64)  | 51  | 4099           | 20 matrices / 26 image jobs in the critic |
|              |              |    |                    |                    |     |                | update: every trunk GEMM of BOTH online   |
|              |              |    |                    |                    |     |                | critics on the split engine; B % 4 != 0   |
| split_ragged | 45 / 45 / 45 | 17 | (256, 128)         | (256, 128)         | 101 | 4099           | ragged first layers (45, 62) stay exact,  |
|              |              |    |                    |                    |     |                | their weight gradients and the later      |
|              |              |    |                    |                    |     |                | layers run on the split engine; dx_cols at|
|              |              |    |                    |                    |     |                | an unaligned base (Oc 45); clipped        |
| many_rows    | 64 / 64 / 64 | 40 | (64)               | (64)               | 21  | 64 num_cus + 37| rows_grid's and bwd_rows_grid's caps,     |
|              |              |    |                    |                    |     |                | fs_concat's 4096 and k_fs_policy_grad's   |
|              |              |    |                    |                    |     |                | 2048 blocks, > 256 loss partials, > 256   |
|              |              |    |                    |                    |     |                | rows in k_fs_alpha_step's strided sum     |

The profiler confirms the engine of every trunk GEMM it sees (net_paths.expected_engines: split-operand engine, `engine` 1, from
4096 rows on for every forward whose in % 4 == 0, every input gradient of a layer l > 0 and every weight gradient; engine 0
everywhere below 4096 rows or with the engine switched off in the context).

Also: acting at A 1, 3, 200, 256 against the oracle and over a row range of a global batch; the two-stream schedule bit for bit at
the ragged act65 shape; rlx_fastsac_replay_sample_f32 on a synthetic ring past one 64-lane pass; rlx_lnmlp_fwd_f32 at a caller-padded
pitch; and a refusal per limit of ln_check / fs_check / the entry points' argument checks, each before any device work.

Measured on the MI355X (split-operand engine on), ||dg|| / ||g|| of the first step's (critic, policy) gradient: narrow 1.4e-7,
2.2e-7; wide 2.8e-6, 2.2e-7; act65 1.5e-6, 4.9e-7; dxlds 1.3e-6, 2.9e-7; split4 3.4e-7, 2.1e-7; split_ragged 8.8e-7, 2.1e-7;
many_rows 2.4e-7, 2.0e-7 ("Shape envelope of FastSAC and FastTD3").

The device's critic gradient error equals a plain float32 evaluation's on the CPU (tests/fastsac_cases.py float32_critic_update:
wide 2.9e-6, act65 1.5e-6, dxlds 1.4e-6, split4 3.8e-7, split_ragged 9.5e-7, many_rows 3.7e-7): it is float32's own, nearly all of it
the categorical projection's bin position at up to 128 atoms.  The cases' learning rate (fastsac_cases.HP) is chosen from that
evaluation: AdamW's step has slope lr / eps on the few entries with |g| within eps of zero, and with the reference's 3e-4 the
float32 evaluation itself leaves `wide`'s critics 1.9e-6 and `dxlds`'s 1.05e-6 from the oracle, past the 1e-6 parameter bar (the
device: 1.58e-6 at `wide`); with 3e-5 it uses a fifth of the bar, and test_fastsac_cases.py holds it to half."""
import ctypes
import re

import numpy as np
import pytest
import torch

import fastsac_cases as fc
import net_paths as npth
from fastsac_cases import _f32, _hp, _rel, _t
from oracle import fastsac as ofs
from rlx_amd.hip import lib as L
from rlx_amd.hip import lnmlp_desc

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
    nc = _num_cus()
    A, NA, B, Op, Oc = c.A, c.NA, c.B, c.Op, c.Oc
    ldc, ldp = npth.pad4(Oc + A), npth.pad4(Op)
    heads = (npth.head_nj(c.ph[-1], 2 * A), npth.head_nj(c.ch[-1], NA))
    dxc = npth.dx_cols_ok(c.ch[0], A)
    cu = npth.trunk_images([(Op, c.ph, False)] + [(Oc + A, c.ch, False)] * 2 + [(Oc + A, c.ch, True)] * 2)
    pu = npth.trunk_images([(Op, c.ph, True)] + [(Oc + A, c.ch, True)] * 2)
    rpb, idle = npth.sample_rows_per_block(A)
    want = {
        "narrow": lambda: len(c.ph) == len(c.ch) == 1 and B == 1 and A == 1 and NA == 2 and heads == (2, 2) and dxc and rpb == 256 and
        c.batch[3][0] > c.h["v_max"] and c.clipped,
        "wide": lambda: max(c.ph + c.ch) == 768 and c.ph[-1] == 704 and heads == (12, 0) and npth.head_masked_threads(704) == 80 and
        16 * (768 + NA) * 4 > 48 * 1024 and NA == 128 and B % 2 == 1 and B < 4096 and dxc,
        "act65": lambda: c.split and Op != Oc and (Oc + A) % 4 != 0 and A > 64 and not dxc and len(c.ch) == 4 and B < 4096 and NA == 65 and
        c.h["max_grad_norm"] > 0 and rpb == 3 and idle == 61,
        "dxlds": lambda: A <= 64 and not dxc and npth.dx_cols_ok(c.ch[0], A - 1) and c.ch[0] == 768 and Oc % 4 != 0 and heads == (4, 8) and
        (Oc + A) % 4 == 0,
        "split4": lambda: B >= 4096 and B % 4 != 0 and cu[:2] == (20, 26) and len(cu[2]) == 20 and pu[:2] == (12, 21) and Op % 4 == 0 and
        (Oc + A) % 4 == 0 and dxc,
        "split_ragged": lambda: B >= 4096 and Op % 4 != 0 and (Oc + A) % 4 != 0 and cu[:2] == (5, 7) and pu[:2] == (3, 6) and dxc and
        Oc % 4 != 0 and npth.bx_dw_usable(True, B, Oc + A, ldc, c.ch[0]) and npth.bx_dw_usable(True, B, Op, ldp, c.ph[0]),
        "many_rows": lambda: npth.rows_grid(nc, B)[1] and npth.bwd_rows_grid(nc, B)[1] and npth.elem_grid(B * ldc)[1] and
        npth.policy_grad_grid(B, A)[1] and npth.div_up(B, 4) > 256 and B > 256 and B >= 4096 and dxc,
    }[name]
    assert want(), (name, heads, dxc, cu[:2], pu[:2], rpb, idle)
    assert name == "many_rows" or B % 4 != 0 or B == 1
    assert cu[1] <= npth.BX_MAX_JOBS and pu[1] <= npth.BX_MAX_JOBS        # no accepted shape leaves a layer without its image


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
    r1 = fc.Run(ctx, dev, c, c.state, eps1, 1, profile=True)
    st1, cmet, pmet, steps = c.twin(c.state, eps1, 1)
    try:
        ratios = fc.check_against_twin(c, r1, st1, cmet, pmet, steps, True, c.state)
    finally:
        (gq_d, gq), (gp_d, gp) = fc.gradient_ratios(c, r1, *steps)
        print(f"FastSAC {name} (B={c.B}) step 1: ||dg||/||g|| critic {_rel(gq_d, gq):.2e}, policy {_rel(gp_d, gp):.2e}")
    _check_engines(ctx, c, r1)
    if c.B >= npth.SPLIT_ROWS:          # what the split engine's operands reach, from the oracle (headroom > 100x, 100x, 10x)
        w = fc.fp16_window(c, c.state, eps1, 1)
        print(f"FastSAC {name}: max |w| {w['weight']:.3g} (< 1023), max |act| {w['act']:.3g} (< 4094), scaled gradient {w['grad_scaled']:.3g} (< 65504)")
        assert w["weight"] * 100 < npth.X_WLIMIT and w["act"] * 100 < npth.X_ALIMIT and 0 < w["grad_scaled"] * 10 < npth.F16_MAX, w
    if c.h["max_grad_norm"] > 0:
        assert cmet[5] > c.h["max_grad_norm"] and pmet[2] > c.h["max_grad_norm"]
    # step 2 from the oracle's state (non-zero moments, bias correction at step 2), rounded to float32 for both sides
    st1 = {k: _f32(v) if np.ndim(v) else float(np.float32(v)) for k, v in st1.items()}
    r2 = c.run(ctx, dev, st1, eps2, 2, key=(3, 4))
    st2, cmet2, pmet2, steps2 = c.twin(st1, eps2, 2)
    m = fc.check_against_twin(c, r2, st2, cmet2, pmet2, steps2, False, st1)
    print(f"FastSAC {name} step 2: ||dm||/||m|| critic {m[0]:.2e}, policy {m[1]:.2e}")
    assert ratios[0] < 1e-5 and ratios[1] < 1e-5


def test_split_engine_off_runs_the_exact_engine(ctx, dev):
    """counter gemm_bx = 0: everything on engine 0 at 4099 rows too, same bars"""
    c = _case("split4")
    eps = c.noise()
    ctx.set_option("gemm_bx", 0)
    try:
        assert ctx.get_counter("gemm_bx") == 0
        r = fc.Run(ctx, dev, c, c.state, eps, 1, profile=True)
        _check_engines(ctx, c, r)
    finally:
        ctx.set_option("gemm_bx", 1)
    st1, cmet, pmet, steps = c.twin(c.state, eps, 1)
    fc.check_against_twin(c, r, st1, cmet, pmet, steps, True, c.state)


# ----------------------------------------------------------------------------------------------------------------------- acting
ACT = {"a1": (181, 300, 7, 1, (64,)), "a3": (182, 257, 9, 3, (128, 64)), "a200": (183, 37, 12, 200, (64,)), "a256": (184, 5, 6, 256, (64, 64))}


@pytest.mark.parametrize("name", list(ACT))
def test_act_matches_the_oracle(ctx, dev, name):
    """k_fs_sample at A 1 (256 rows per block), A 3 (85 rows, the last thread idle), A 200 and A 256 (one row per block): sampled
    with injected noise and deterministic, against the oracle at 1e-5; the key is split only when something is drawn"""
    seed, N, O, A, hidden = ACT[name]
    rng = np.random.default_rng(seed)
    rpb, idle = npth.sample_rows_per_block(A)
    assert {"a1": (256, 0), "a3": (85, 1), "a200": (1, 56), "a256": (1, 0)}[name] == (rpb, idle)
    p, _ = ofs.make_params(seed, O, A, 21, policy_hidden=hidden, critic_hidden=(64,))
    pd = lnmlp_desc(O, hidden, 2 * A)
    obs, eps = _f32(rng.standard_normal((N, O))), _f32(rng.standard_normal((N, A)))
    scale = _f32(np.linspace(0.5, 1.5, A))
    hp = _hp(fc.HP, 21, False)
    P, x, sc = _t(p, dev), _t(obs, dev), _t(scale, dev)
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    mean, ls = ofs.policy_forward(T(p), O, A, T(obs), fc.HP["log_std_min"], fc.HP["log_std_max"], hidden)
    act = torch.full((N, A), 1234.5, device=dev)
    key = L.prng_key(4)
    te = _t(eps, dev)
    ctx.dbg_set_sac_noise(te, None)
    try:
        ctx.fastsac_act(pd, P, x, sc, key, act, hp)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    ea, _ = ofs.sample(mean, ls, T(eps), T(scale))
    assert _rel(act.cpu().numpy(), ea.numpy()) < 1e-5
    k1 = ctx.fastsac_act(pd, P, x, sc, key, act, hp, deterministic=True)
    assert np.array_equal(k1, key)                       # nothing drawn: the key is untouched
    da, _ = ofs.sample(mean, ls, torch.zeros_like(mean), T(scale))
    assert _rel(act.cpu().numpy(), da.numpy()) < 1e-5


def test_act_on_a_row_range_equals_the_rows_of_the_full_call(ctx, dev):
    """the library's own draws: rows [r0, r0 + N) with row_offset = r0, n_global = NG are bit for bit the rows of the NG-row call"""
    seed, NG, O, A, hidden = 185, 301, 9, 3, (64,)
    rng = np.random.default_rng(seed)
    p, _ = ofs.make_params(seed, O, A, 21, policy_hidden=hidden, critic_hidden=(64,))
    pd, hp = lnmlp_desc(O, hidden, 2 * A), _hp(fc.HP, 21, False)
    P, x, sc = _t(p, dev), _t(rng.standard_normal((NG, O)), dev), _t(np.linspace(0.5, 1.5, A), dev)
    full = torch.empty(NG, A, device=dev)
    key = L.prng_key(9)
    k_full = ctx.fastsac_act(pd, P, x, sc, key, full, hp)
    assert not np.array_equal(k_full, key) and full.std().item() > 0.05
    for r0, n in ((0, 86), (86, 170), (256, 45)):
        part = torch.empty(n, A, device=dev)
        k = ctx.fastsac_act(pd, P, x[r0:r0 + n].contiguous(), sc, key, part, hp, row_offset=r0, n_global=NG)
        assert np.array_equal(k, k_full) and torch.equal(part, full[r0:r0 + n]), r0


# ---------------------------------------------------------------------------------------------------------- two-stream schedule
def test_two_stream_schedule_is_bit_identical_at_a_ragged_shape(ctx, dev):
    """two_streams 0 against 1 at act65: critic_states, ragged Oc + A, the whole-GEMM first_layer_dx"""
    c = _case("act65")
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


# ------------------------------------------------------------------------------------------------------------------ replay ring
@pytest.mark.parametrize("tag,n_steps,full", [("n1", 1, True), ("n3_partial", 3, False), ("n3_full", 3, True), ("n_capacity", 6, True)])
def test_replay_sample_on_a_synthetic_ring(ctx, dev, tag, n_steps, full):
    """O 70 and A 65 (both past one 64-lane pass), windows that wrap, n_steps == capacity, a full ring whose newest row is not
    done (it counts as truncated), B % 4 != 0: against oracle.fastsac.nstep_sample"""
    rng = np.random.default_rng(191)
    cap, ne, O, A, B, gamma = 6, 5, 70, 65, 203, 0.97
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    ring = dict(states=f(cap, ne, O), next_states=f(cap, ne, O), actions=f(cap, ne, A), rewards=f(cap, ne),
                dones=(rng.random((cap, ne)) < 0.25).astype(np.float32), truncations=(rng.random((cap, ne)) < 0.15).astype(np.float32))
    pos, size = (2, cap) if full else (4, 4)
    last = (pos - 1) % cap
    ring["dones"][last, :3] = 0.0                       # the newest row: not done in some envs, done in others
    ring["truncations"][last, :3] = 0.0
    ring["dones"][last, 3:] = 1.0
    if full:
        idx_t = rng.integers(0, cap, B)                 # windows wrap past the end of the ring
        idx_t[:cap] = np.arange(cap)
    else:
        idx_t = rng.integers(0, size - n_steps + 1, B)
    idx_e = rng.integers(0, ne, B)
    exp = ofs.nstep_sample({k: v.astype(np.float64) for k, v in ring.items()}, pos, size, cap, n_steps, gamma, idx_t, idx_e)
    names = ("states", "next_states", "actions", "rewards", "dones", "truncations")
    dring = tuple(_t(ring[k], dev) for k in names)
    out = (torch.empty(B, O, device=dev), torch.empty(B, O, device=dev), torch.empty(B, A, device=dev)) + tuple(
        torch.empty(B, device=dev) for _ in range(4))
    ctx.fastsac_replay_sample(dring, n_steps, gamma, pos, size, _t(idx_t, dev, np.int32), _t(idx_e, dev, np.int32), out)
    # the n-step return: n terms r gamma^k, each with powf (2 ulp), one product and one running sum in float32, against float64;
    # everything else is a copy or a sum of 0 / 1 masks: exact
    atol = n_steps * 4 * 2.0 ** -24 * np.abs(ring["rewards"]).max()
    for name, got, e in zip(names + ("effective_n_steps",), out, exp):
        if name == "rewards":
            np.testing.assert_allclose(got.cpu().numpy(), e, rtol=0, atol=atol, err_msg=tag + " " + name)
        else:
            assert np.array_equal(got.cpu().numpy().astype(np.float64), e), tag + " " + name
    if full and n_steps > 1:                            # the rule is exercised: some window ends on the newest, not-done row
        assert np.any((exp[5] > 0) & (exp[4] == 0))


# ---------------------------------------------------------------------------------------------------------------- lnmlp forward
def test_lnmlp_fwd_at_a_caller_padded_pitch(ctx, dev):
    """ldx a multiple of 4 greater than in_dim (the rows are used in place; the padding holds zeros as the header asks)"""
    rng = np.random.default_rng(192)
    M, O, ld, hidden, out = 77, 45, 52, (128, 64), 11
    _, q = ofs.make_params(192, O - 3, 3, out, policy_hidden=(64,), critic_hidden=hidden)
    d = lnmlp_desc(O, hidden, out)
    x = np.zeros((M, ld), np.float32)
    x[:, :O] = rng.standard_normal((M, O)).astype(np.float32)
    got = ctx.lnmlp_fwd(d, _t(q[0], dev), _t(x, dev), torch.empty(M, out, device=dev)).cpu().numpy()
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    exp = ofs.forward(T(q[0]), O, hidden, out, T(x[:, :O])).numpy()
    assert _rel(got, exp) < 1e-5
    tight = ctx.lnmlp_fwd(d, _t(q[0], dev), _t(x[:, :O], dev), torch.empty(M, out, device=dev)).cpu().numpy()
    assert np.array_equal(got, tight)


# --------------------------------------------------------------------------------------------------------------------- refusals
EINVAL, EUNSUP = -1, -4
SENTINEL = 1234.5
GOOD = dict(O=8, A=3, ph=(64, 64), ch=(64, 64), NA=21, B=12)


def _refusals():
    """(name, overrides, code, message fragment, entry points).  Overrides: pd / qd = (in_dim, hidden, out_dim) of the policy /
    critic descriptor, hparams by name, cs / cn = pass critic_states / critic_next_states, rows, n_global"""
    O, A, NA = GOOD["O"], GOOD["A"], GOOD["NA"]
    all3, upd, act = ("critic", "policy", "act"), ("critic", "policy"), ("act",)
    pd = lambda hidden, out=2 * A: dict(pd=(O, hidden, out))
    qd = lambda hidden, i=O + A, out=NA: dict(qd=(i, hidden, out))
    wmsg = "multiples of 64, at most 768"
    return [
        ("policy_0_layers", pd(()), EINVAL, "1..4 hidden layers", all3),
        ("policy_5_layers", pd((64,) * 5), EINVAL, "1..4 hidden layers", all3),
        ("critic_0_layers", qd(()), EINVAL, "1..4 hidden layers", upd),
        ("critic_5_layers", qd((64,) * 5), EINVAL, "1..4 hidden layers", upd),
        ("policy_width_0", pd((64, 0)), EUNSUP, wmsg, all3),
        ("policy_width_96", pd((96, 64)), EUNSUP, wmsg, all3),
        ("policy_width_832", pd((832,)), EUNSUP, wmsg, all3),
        ("critic_width_0", qd((0,)), EUNSUP, wmsg, upd),
        ("critic_width_96", qd((64, 96)), EUNSUP, wmsg, upd),
        ("critic_width_832", qd((832, 64)), EUNSUP, wmsg, upd),
        ("policy_out_odd", pd((64, 64), 2 * A + 1), EINVAL, "2 * act_dim", all3),
        ("policy_out_0", pd((64, 64), 0), EINVAL, "positive widths", all3),
        ("critic_in_is_act", qd((64, 64), A), EINVAL, "critic in_dim = critic obs + act", upd),
        ("critic_out_not_atoms", qd((64, 64), O + A, NA + 1), EINVAL, "out_dim = nr_atoms", upd),
        ("atoms_1", dict(qd=(O + A, (64, 64), 1), nr_atoms=1), EINVAL, "nr_atoms (2..128)", upd),
        ("atoms_129", dict(qd=(O + A, (64, 64), 129), nr_atoms=129), EINVAL, "nr_atoms (2..128)", upd),
        ("v_equal", dict(v_min=5.0, v_max=5.0), EINVAL, "v_max > v_min", upd),
        ("v_below", dict(v_min=5.0, v_max=-5.0), EINVAL, "v_max > v_min", upd),
        ("log_std_equal", dict(log_std_min=-2.0, log_std_max=-2.0), EINVAL, "log_std_max > log_std_min", upd),
        ("critic_width_without_critic_states", qd((64, 64), O + A + 2), EINVAL, "needs critic_states", upd),
        ("only_critic_states", dict(cs=True), EINVAL, "critic_states AND critic_next_states", ("critic",)),
        ("only_critic_next_states", dict(cn=True), EINVAL, "critic_states AND critic_next_states", ("critic",)),
        ("rows_0", dict(rows=0), EINVAL, "bad args", all3),
        ("n_global_below_n", dict(n_global=GOOD["B"] - 1), EINVAL, "bad args", act),
    ]


REFUSALS = [(e, r) for r in _refusals() for e in r[4]]


@pytest.mark.parametrize("entry,r", REFUSALS, ids=["%s-%s" % (e, r[0]) for e, r in REFUSALS])
def test_envelope_refusals(ctx, dev, entry, r):
    """a value just outside each limit: the documented code (RlxError), rlx_last_error() names it, and nothing is written (outputs
    prefilled with a sentinel; parameters, moments, log_alpha, the key and the count unchanged); the context then runs a valid call"""
    name, over, code, msg, _ = r
    O, A, NA, B = GOOD["O"], GOOD["A"], GOOD["NA"], GOOD["B"]
    c = fc.Case(195, O, A, GOOD["ph"], GOOD["ch"], NA, B)
    pd = lnmlp_desc(*over["pd"]) if "pd" in over else c.pd
    qd = lnmlp_desc(*over["qd"]) if "qd" in over else c.qd
    h = dict(c.h, **{k: v for k, v in over.items() if k in c.h})
    hp = _hp(h, over.get("nr_atoms", NA), False)
    rows = over.get("rows", B)
    key = L.prng_key(3)
    key0 = key.copy()
    fill = lambda *sh: torch.full(sh, SENTINEL, device=dev)
    st = {k: _t(np.atleast_1d(c.state[k]), dev) for k in fc.STATE_KEYS}
    for k in ("pm", "pv", "qm", "qv", "am", "av"):
        st[k].fill_(SENTINEL)
    before = {k: v.clone() for k, v in st.items()}
    batch = tuple(_t(x, dev) for x in c.batch)          # valid buffers whatever `rows` says: the row count alone decides
    scale = _t(c.scale, dev)
    extra = fill(B, O + 2)
    lib = L.load_library()
    cnt = ctypes.c_int64(5)
    karr = (ctypes.c_uint32 * 2)(int(key[0]), int(key[1]))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    if entry == "act":
        outs = [fill(B, A)]
        rc = lib.rlx_fastsac_act_f32(ctx.h, ctypes.byref(pd), ptr(st["P"]), ptr(batch[0]), ptr(scale), karr, L.THREEFRY_PARTITIONABLE,
                                     ptr(outs[0]), rows, 0, 0, over.get("n_global", rows), ctypes.byref(hp), None)
    elif entry == "critic":
        outs = [fill(8)]
        cs = ptr(extra) if over.get("cs") else None
        cn = ptr(extra) if over.get("cn") else None
        rc = lib.rlx_fastsac_critic_update_f32(
            ctx.h, ctypes.byref(pd), ptr(st["P"]), ctypes.byref(qd), ptr(st["Q"]), ptr(st["qm"]), ptr(st["qv"]), ptr(st["QT"]), ptr(st["la"]),
            ptr(st["am"]), ptr(st["av"]), ptr(batch[0]), ptr(batch[1]), cs, cn, *[ptr(x) for x in batch[2:]], ptr(scale), rows, karr,
            L.THREEFRY_PARTITIONABLE, ctypes.byref(cnt), ctypes.byref(hp), ptr(outs[0]), None)
    else:
        outs = [fill(3)]
        rc = lib.rlx_fastsac_policy_update_f32(
            ctx.h, ctypes.byref(pd), ptr(st["P"]), ptr(st["pm"]), ptr(st["pv"]), ctypes.byref(qd), ptr(st["Q"]), ptr(st["la"]), ptr(batch[0]),
            None, ptr(scale), rows, karr, L.THREEFRY_PARTITIONABLE, ctypes.byref(cnt), ctypes.byref(hp), ptr(outs[0]), None)
    assert rc == code, (name, rc)
    assert msg in lib.rlx_last_error().decode(), lib.rlx_last_error().decode()
    with pytest.raises(L.RlxError) as e:                 # the binding raises the same code and message
        L._check(rc, "rlx_fastsac")
    assert int(re.search(r"rc=(-?\d+)", str(e.value)).group(1)) == code and msg in str(e.value)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), name
    for k in fc.STATE_KEYS:
        assert torch.equal(st[k], before[k]), (name, k)
    assert (karr[0], karr[1]) == (int(key0[0]), int(key0[1])) and cnt.value == 5
    # the context still serves a valid call
    good = fc.Case(196, O, A, GOOD["ph"], GOOD["ch"], NA, B)
    g = good.run(ctx, dev, good.state, good.noise(), 1)
    assert np.all(np.isfinite(g.cmetrics)) and np.all(np.isfinite(g.pmetrics)) and g.cmetrics[0] > 0
