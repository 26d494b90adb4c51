"""GPU: rlx_redq_update_f32, rlx_aqe_update_f32, rlx_droq_update_f32 and rlx_tqc_update_f32 (redq.hip's redq_loop, tqc.hip, sac_ens.hip)
across the shape envelope ens_check_net / ens_prologue accept, against each algorithm's float64 twin at the bars of its own file
(test_gpu_redq.py BARS and check, test_gpu_aqe.py, test_gpu_droq.py; test_gpu_tqc.py check_first_step).  tests/ens_cases.py holds
the case table; nc = num_cus of the device:

| case         | O / Oc  | A            | policy hidden  | critic hidden (DroQ)           | E, M                    | G | B          | AQE H, dropped | TQC N, dropped per net |
|--------------|---------|--------------|----------------|--------------------------------|-------------------------|---|------------|----------------|------------------------|
| narrow       | 5 / 5   | 1            | (64)           | (64)                           | 2, 1                    | 2 | 1          | 1, 1           | 2, 1                   |
| wide         | 48 / 48 | 16 (DroQ 27) | (1024, 128)    | (1024, 768) ((768, 704))       | 2, 2                    | 1 | 37         | 8, 3           | 25, 2                  |
| act64        | 70 / 29 | 64           | (128, 64, 64)  | (128, 64, 64) ((128, 320, 64)) | 3, 2 (AQE E 16; TQC E 4) | 2 | 37         | 8, 100         | 32, 3                  |
| split_ragged | 45 / 45 | 17           | (256, 128)     | (256, 128)                     | 2, 2                    | 2 | 4099       | 3, 2           | 25, 2                  |
| cut_inside   | 8 / 9   | 3            | (64, 128, 192) | (64, 128, 192)                 | 6, 2                    | 1 | 4099       | 2, 3           | 5, 1                   |
| many_rows    | 64 / 64 | 40           | (64)           | (64)                           | 2, 2                    | 1 | 64 nc + 37 | 40, 5          | 40, 3                  |

  narrow        one row, one hidden layer, A 1 (k_ens_sample / k_ens_policy_grad: 256 rows a block); AQE T 2 with K 1, TQC T 4
  wide          width 1024; first_layer_dx through the whole GEMM at the smallest A at which dx_cols_ok fails (16 at first width 1024,
                DroQ 27 at 768), k_ens_policy_grad reading the columns [Oc, Oc + A) of it at pitch ldc; critic head K 768 with one output
                untiled by 64 bytes of LDS, DroQ's K 704 tiled with 80 masked threads; DroQ's D > 256 block form in both layers
  act64         A 64 (four rows a block), dx_cols with 64 columns at the unaligned base Oc 29, Oc + A = 93 ragged, policy head N 128,
                DroQ's wide block form in the middle layer, AQE and TQC at T 128 (both sort slots full), G 2 at unaligned batch offsets
  split_ragged  the split-operand engine above width 64 at B % 4 != 0; the ragged first layers (45, 62) stay exact while their weight
                gradients go split; the images rebuilt between the two critic steps
  cut_inside    the image list ends INSIDE a network (REDQ / DroQ: online critic 4 in the critic step, critic 5 in the policy step):
                one layer of it runs on the split-operand engine and the next on the exact one, forward and backward; A 3 (one idle lane)
  many_rows     rows_grid's and bwd_rows_grid's caps, fs_concat's and k_ens_fill's 4096 blocks, more than 256 rows in the single-block
                sums of k_ens_mean / k_ens_finish; A 40 (24 idle lanes); AQE and TQC at T 80 (second sort slot partly filled)

test_ens_cases.py recomputes these claims from tests/net_paths.py, holds each case's float32 twin to half of every bar and shows
that the bars see a dropped tail row, a zeroed last action column and a last critic on its neighbour's parameters.

One update call per case with injected noise, the library's own target subsets (REDQ, DroQ) and the Python restatement of the
dropout mask stream (DroQ).  The bars are the one-step bars: for G 2 and the cases of 4099 rows and more the rule max(bar, 2 F32_GAP)
(ens_cases.F32_GAP) leaves every one of them where it is.  TQC's critic gradient at 4099 rows and more may go through
admissible_critic_gradient under its MAX_FLIPS, as test_update_split_operand_engine's does.

Measured on the MI355X (split-operand engine on), the largest figure over the six cases (bars 1e-5, 1e-5, 1e-5, 6.0e-4): REDQ pm 4.7e-7,
qm 3.3e-7, norms 1.6e-7, Qmax 7.5e-7; AQE 4.9e-7, 3.3e-7, 2.3e-7, 3.9e-5; DroQ 5.0e-7, 7.0e-7, 2.1e-7, 6.5e-7; TQC 5.0e-7, 6.3e-7, 1.4e-7,
6.9e-6, with no kink flip taken ("Shape envelope of the ensemble-SAC family", has every case)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ens_cases as ec
import net_paths as npth
from oracle import nets
from rlx_amd.hip import lib as L
from rlx_amd.hip import AqeHparams, DroqHparams, RedqHparams, RlxError, TqcHparams, mlp_desc

pytestmark = pytest.mark.gpu

CASES = [(a, n) for a in ec.ALGOS for n in ec.NAMES]
IDS = [f"{a}-{n}" for a, n in CASES]
GAMMA, TAU, LR = ec.m_redq.GAMMA, ec.m_redq.TAU, ec.m_redq.LR


@functools.lru_cache(maxsize=None)
def _case(algo, name):
    return ec.shape_case(algo, name, torch.cuda.get_device_properties(0).multi_processor_count)


def _steps(c):
    args = (c.O, c.ph, c.Oc + c.A, c.qh, c.E, c.M)
    if c.algo == "tqc":
        return [npth.ens_nets("tqc", "update", *args)]
    return [npth.ens_nets(c.algo, "critic", *args)] * c.G + [npth.ens_nets(c.algo, "policy", *args)]


def _run_and_check(ctx, dev, c, prof=False):
    """one update against the float64 twin at the file's own bars; the key chain, the counters and the subsets as its own tests do"""
    if c.algo != "tqc":
        return c.mod._run_and_check(ctx, dev, c.c, 1, prof)[1]
    m, t = ec.m_tqc, c.c
    r = m.Run(ctx, dev, t, t.state, ec.KEY, 1, inject=t.eps, prof=prof)
    assert np.array_equal(r.key, c.tqc_key()) and r.count == 1
    new, met, grads, aux = t.twin(t.state, t.eps)
    f = c.figures(r.out, r.metrics, new, met)
    print(f"tqc update {c.name}: " + " ".join(f"{k} {v:.2e}/{ec.BARS[k]:.1e}" for k, v in f.items()))
    if c.B >= npth.SPLIT_ROWS:
        grads = (grads[0], m.admissible_critic_gradient(t, r, grads[1], aux, c.name), grads[2])
    m.check_first_step(r, new, met, grads, c.name)
    return r


@pytest.mark.parametrize("algo,name", CASES, ids=IDS)
def test_update_matches_the_twin(ctx, dev, algo, name):
    c = _case(algo, name)
    assert c.bars() == ec.BARS
    r = _run_and_check(ctx, dev, c)
    assert r.metrics[9] == 0.0 and all(np.all(np.isfinite(v)) for v in r.out.values())


@pytest.mark.parametrize("name", ["split_ragged", "cut_inside"])
@pytest.mark.parametrize("algo", ec.ALGOS)
def test_engines(ctx, dev, algo, name):
    """every profiled trunk GEMM row against the mirror's launch counts per engine.  At cut_inside the shape of the layer at which
    the image list ends shows on both engines"""
    c = _case(algo, name)
    bx = ctx.get_counter("gemm_bx") == 1
    c.run(ctx, dev, prof=True)
    rows = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    print(f"{algo} {name} gemm rows:", sorted((q["kernel"], q["engine"], q["M"], q["N"], q["K"], q["launches"]) for q in rows))
    exp = npth.expected_engine_counts(_steps(c), bx, c.B, c.A)
    npth.check_engine_counts(rows, exp)
    if not bx:
        assert all(q["engine"] == 0 for q in rows), rows
    elif name == "cut_inside":
        _, l = npth.image_cut(_steps(c)[0])
        seen = {q["engine"] for q in rows if (q["kernel"], q["M"], q["N"], q["K"]) == ("k_gemm_fwd", c.B, c.qh[l], c.qh[l - 1])}
        assert seen == {0, 1} and set(exp[("k_gemm_fwd", c.B, c.qh[l], c.qh[l - 1])]) == {0, 1}, (seen, l)


@pytest.mark.parametrize("algo", ec.ALGOS)
def test_two_identical_calls_give_identical_bits(ctx, dev, algo):
    for name in ("act64", "split_ragged"):
        c = _case(algo, name)
        assert c.run(ctx, dev, inject=False).same_bits(c.run(ctx, dev, inject=False)), name
        assert c.run(ctx, dev).same_bits(c.run(ctx, dev)), name


@pytest.mark.parametrize("algo", ["redq", "droq"])
def test_split_engine_off_meets_the_same_bars(ctx, dev, algo):
    """gemm_bx 0: everything on the exact engine at 4099 rows too, same bars"""
    c = _case(algo, "split_ragged")
    was = ctx.get_counter("gemm_bx")
    ctx.set_option("gemm_bx", 0)
    try:
        assert ctx.get_counter("gemm_bx") == 0
        _run_and_check(ctx, dev, c, prof=True)
        rows = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
        assert rows and all(q["engine"] == 0 for q in rows), rows
        npth.check_engine_counts(rows, npth.expected_engine_counts(_steps(c), False, c.B, c.A))
    finally:
        ctx.set_option("gemm_bx", was)


# ----------------------------------------------------------------------------------------------------------------------- refusals
def _hp(algo, E=2, G=2):
    if algo == "redq":
        return RedqHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, 0.0, LR, 0.9, 0.999, 1e-8, E, 2, G)
    if algo == "aqe":
        return AqeHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, 0.0, LR, 0.9, 0.999, 1e-8, E, 2, 2, G)
    if algo == "droq":
        hp = DroqHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, 0.0, LR, 0.9, 0.999, 1e-8, E, 2, G)
        hp.dropout_rate = 0.25
        return hp
    return TqcHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, LR, 0.9, 0.999, 1e-8, 1.0, E, 25, 2)


REFUSALS = [(a, w) for a in ec.ALGOS for w in ("p_layers0", "q_layers0", "p_layers4", "q_layers4", "p_width1088", "q_width1088", "b0")]
REFUSALS += [(a, "a65") for a in ("redq", "aqe", "droq")] + [("droq", "q_width832")]
WANT = {"layers0": (-1, "1..3 hidden layers"), "layers4": (-1, "1..3 hidden layers"), "width1088": (-4, "at most 1024"), "a65": (-4, "act_dim"),
        "width832": (-4, "at most 768"), "b0": (-1, "B must be positive")}


@pytest.mark.parametrize("algo,what", REFUSALS, ids=[f"{a}-{w}" for a, w in REFUSALS])
def test_refusals(ctx, dev, algo, what):
    """outside the envelope: the documented code and message, nothing written, and the context serves a valid call afterwards"""
    O, A, G = 8, 2, 2
    which, kind = what.split("_") if "_" in what else ("", what)
    hidden = {"layers0": [], "layers4": [64, 64, 64, 64], "width1088": [64, 1088], "width832": [64, 832]}.get(kind, [64, 64])
    if kind == "a65":
        A = 65
    qout = {"redq": 1, "droq": 1, "aqe": 2, "tqc": 25}[algo]
    pd = mlp_desc(O, hidden if which == "p" else [64, 64], 2 * A, nets.ACT_RELU, False, False)
    qd = mlp_desc(O + A, hidden if which == "q" else [64, 64], qout, nets.ACT_RELU, False, False)
    x = torch.zeros(64, device=dev)
    rows = x[:1] if kind == "b0" else x          # redq_loop's B is rewards.numel() / G, TQC's is actions.shape[0]
    key = np.array(ec.KEY, np.uint32)
    code, word = WANT[kind]
    if (algo, what) == ("droq", "q_width1088"):          # DroQ's own, narrower limit on its critics answers first
        word = "at most 768"
    with pytest.raises(RlxError) as e:
        if algo == "tqc" and kind == "b0":       # (the binding takes B from actions.shape[0], and an empty tensor has no pointer)
            p, hp, cnt = L._ptr(x, torch.float32), _hp(algo), ctypes.c_int64(0)
            L._check(ctx.lib.rlx_tqc_update_f32(ctx.h, ctypes.byref(pd), p, p, p, ctypes.byref(qd), p, p, p, p, p, p, p, p, p, p, p, p,
                                                ctypes.c_int64(0), L._key_arr(key), 1, ctypes.byref(cnt), ctypes.byref(hp), p, L._stream()),
                     "rlx_tqc_update_f32")
        elif algo == "tqc":
            ctx.tqc_update(pd, x, x, x, qd, x, x, x, x, x, x, x, (x, x, x, x, x), key, 0, _hp(algo), x)
        else:
            getattr(ctx, algo + "_update")(pd, x, x, x, qd, x, x, x, x, x, x, x, (x, x, x, rows, x), key, 0, 0, _hp(algo, G=G), x)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(x).item() == 0
    r = _case(algo, "narrow").run(ctx, dev)
    assert r.metrics[9] == 0.0 and np.all(np.isfinite(r.metrics)) and np.any(r.out["Q"] != _case(algo, "narrow").c.state["Q"].astype(np.float32))
