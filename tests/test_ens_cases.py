"""CPU: the shape cases of test_gpu_ens_shapes.py (tests/ens_cases.py) before any device sees them.

  - every path the case table names is recomputed from the mirror of the host selection code (tests/net_paths.py, num_cus 256),
    where the image builder's job table cuts included;
  - every case's twin in numpy float32 is within half of each one-step bar of the float64 twin (the second moments: float32's
    1 - 0.999 against 0.001, 1.3e-5 under their 5e-5), so a miss on the device is a kernel's and not the inputs';
  - the bars see a wrong tail: the float64 twin with the last batch row left out of the critic gradient, with the last action
    column of dQ/da zeroed, or with the last critic evaluated on its neighbour's parameters misses the bar of the quantity that
    fault lands in by more than a factor of ten, and leaves exact what it cannot reach."""
import functools

import numpy as np
import pytest

import ens_cases as ec
import net_paths as npth

CASES = [(a, n) for a in ec.ALGOS for n in ec.NAMES]
IDS = [f"{a}-{n}" for a, n in CASES]
NC = 256


@functools.lru_cache(maxsize=None)
def _case(algo, name):
    return ec.shape_case(algo, name, NC)


@functools.lru_cache(maxsize=None)
def _reference(algo, name):
    """(extras, new state, metrics) of the float64 twin: computed once, read by every test of the case"""
    c = _case(algo, name)
    ex = c.extras()
    new, met = c.twin(ex)[:2]
    return ex, new, met


def _steps(c):
    """the image lists of one call, in order: G critic steps and the policy step, or TQC's one"""
    args = (c.O, c.ph, c.Oc + c.A, c.qh, c.E, c.M)
    if c.algo == "tqc":
        return [npth.ens_nets("tqc", "update", *args)]
    return [npth.ens_nets(c.algo, "critic", *args)] * c.G + [npth.ens_nets(c.algo, "policy", *args)]


def test_the_mirrors_of_the_lane_and_block_selection():
    assert [npth.ens_lanes_per_row(a) for a in (1, 2, 3, 4, 5, 17, 32, 33, 40, 63, 64)] == [1, 2, 4, 4, 8, 32, 32, 64, 64, 64, 64]
    assert npth.ens_sample_rows_per_block(1) == (256, 0) and npth.ens_sample_rows_per_block(40) == (4, 24)
    assert [npth.drop_ln_relu_form(d) for d in (64, 256, 320, 768)] == [4, 4, 12, 12]
    # dx_cols_ok fails from A 16 at width 1024 and from A 27 at width 768
    assert npth.dx_cols_ok(1024, 15) and not npth.dx_cols_ok(1024, 16) and npth.dx_cols_ok(768, 26) and not npth.dx_cols_ok(768, 27)
    # fs_head_bwd with one output: K 768 misses the tiled kernel's 48 KB by 64 bytes, K 704 is tiled with 80 idle threads, K 1024 untiled
    assert 16 * (768 + 1) * 4 - 48 * 1024 == 64 and npth.head_nj(768, 1) == 0 and npth.head_nj(1024, 1) == 0
    assert npth.head_nj(704, 1) == 2 and npth.head_masked_threads(704) == 80
    # N = 2 A = 128: tiled at K 64 and 128, untiled from K 256 on (nj > 12)
    assert npth.head_nj(64, 128) == 4 and npth.head_nj(128, 128) == 8 and npth.head_nj(256, 128) == 0


@pytest.mark.parametrize("algo,name", CASES, ids=IDS)
def test_shape_case_reaches_its_paths(algo, name):
    """the case table's claims, from the host selection code's arithmetic"""
    c = _case(algo, name)
    A, B, O, Oc, E, G, ph, qh = c.A, c.B, c.O, c.Oc, c.E, c.G, c.ph, c.qh
    loop, droq = algo != "tqc", algo == "droq"
    T = E * c.heads
    ldc, ldp = npth.pad4(Oc + A), npth.pad4(O)
    rpb, idle = npth.ens_sample_rows_per_block(A)
    dxc = npth.dx_cols_ok(qh[0], A)
    steps = _steps(c)
    cuts = [npth.image_cut(s) for s in (steps[0], steps[-1])]
    forms = [npth.drop_ln_relu_form(w) for w in qh] if droq else []
    counts = npth.expected_engine_counts(steps, True, B, A)
    both = {k for k, v in counts.items() if len(v) == 2}
    dropped = {"aqe": getattr(c.c, "dropped", 0), "tqc": E * getattr(c.c, "dropped", 0)}.get(algo, 0)

    def narrow():
        return B == 1 and len(ph) == len(qh) == 1 and A == 1 and (rpb, idle) == (256, 0) and dxc and (not loop or G == 2) and \
            {"aqe": (T, T - dropped) == (2, 1), "tqc": T == 4}.get(algo, True)

    def wide():
        w0, a0 = (768, 27) if droq else (1024, 16)
        head = (qh[-1] == 704 and npth.head_nj(704, 1) == 2 and npth.head_masked_threads(704) == 80 and forms == [12, 12]) if droq else \
            (qh[-1] == 768 and npth.head_nj(768, c.heads) == 0)
        return max(ph) == 1024 and (qh[0], A) == (w0, a0) and not dxc and npth.dx_cols_ok(w0, A - 1) and head and B < 4096 and B % 4 != 0 and \
            (algo != "redq" or 16 * (768 + c.heads) * 4 - 48 * 1024 == 64)

    def act64():
        return A == 64 and (rpb, idle) == (4, 0) and dxc and c.asym and Oc == 29 and Oc % 4 != 0 and Oc + A == 93 and 2 * A == 128 and \
            npth.head_nj(ph[-1], 2 * A) == 4 and B < 4096 and (not droq or forms == [4, 12, 4]) and (algo not in ("aqe", "tqc") or T == 128) and \
            (not loop or (G == 2 and B % 4 != 0 and (B * Oc) % 4 != 0 and (B * O) % 4 != 0))

    def split_ragged():
        hidden = {k: v for k, v in counts.items() if k[0] == "k_gemm_fwd" and k[3] % 4 == 0}
        ragged = {k: v for k, v in counts.items() if k[0] == "k_gemm_fwd" and k[3] % 4 != 0}
        dws = {k: v for k, v in counts.items() if k[0] == "k_gemm_dw"}
        return B >= 4096 and B % 4 != 0 and min(ph + qh) > 64 and (O, Oc + A) == (45, 62) and cuts == [None, None] and not both and dxc and \
            Oc % 4 != 0 and hidden and all(set(v) == {1} for v in hidden.values()) and {k[3] for k in ragged} == {45, 62} and \
            all(set(v) == {0} for v in ragged.values()) and all(set(v) == {1} for v in dws.values()) and {k[1] for k in dws} >= {45, 62} and \
            npth.bx_dw_usable(True, B, Oc + A, ldc, qh[0]) and npth.bx_dw_usable(True, B, O, ldp, ph[0]) and (not loop or G == 2)

    def cut_inside():
        # (net index in the step's list, layer): REDQ / DroQ cut inside online critic 4 in the critic step (1 policy + 2 targets in front
        # of it) and inside critic 5 in the policy step; AQE lists all 6 targets; TQC has one list: policy, 6 online, 6 targets
        want = {"redq": [(1 + 2 + 4, 2), (1 + 5, 1)], "droq": [(1 + 2 + 4, 2), (1 + 5, 1)], "aqe": [(1 + 6 + 2, 1), (1 + 5, 1)],
                "tqc": [(1 + 5, 1), (1 + 5, 1)]}[algo]
        shapes = {("k_gemm_fwd", B, qh[l], qh[l - 1]) for _, l in want}
        return B >= 4096 and O % 4 == 0 and (Oc + A) % 4 == 0 and c.asym and len(qh) == 3 and cuts == want and all(l > 0 for _, l in want) and \
            shapes <= both and (A, npth.ens_lanes_per_row(A), idle) == (3, 4, 1) and npth.trunk_images([n[:3] for n in steps[0]])[1] <= npth.BX_MAX_JOBS

    def many_rows():
        return npth.rows_grid(NC, B)[1] and npth.bwd_rows_grid(NC, B)[1] and npth.elem_grid(B * ldc)[1] and npth.elem_grid(B * ldp)[1] and \
            (algo != "aqe" or npth.elem_grid(E * B * c.heads)[1]) and B > 256 and B >= 4096 and (A, rpb, idle) == (40, 4, 24) and \
            (algo not in ("aqe", "tqc") or T == 80) and cuts == [None, None]

    ok = {"narrow": narrow, "wide": wide, "act64": act64, "split_ragged": split_ragged, "cut_inside": cut_inside, "many_rows": many_rows}[name]()
    assert ok, (algo, name, rpb, idle, dxc, cuts, forms, sorted(both))
    assert (c.O != c.Oc) == c.asym and E <= 16 and T <= 128 and 1 <= len(qh) <= 3 and max(qh) <= (768 if droq else 1024)


def test_engine_counts_without_the_split_engine_and_below_4096_rows():
    for algo in ec.ALGOS:
        c = _case(algo, "cut_inside")
        off = npth.expected_engine_counts(_steps(c), False, c.B, c.A)
        on = npth.expected_engine_counts(_steps(c), True, c.B, c.A)
        assert all(set(v) == {0} for v in off.values()) and set(off) == set(on)
        assert {k: sum(v.values()) for k, v in off.items()} == {k: sum(v.values()) for k, v in on.items()}
        small = npth.expected_engine_counts(_steps(_case(algo, "act64")), True, 37, 64)
        assert small and all(set(v) == {0} for v in small.values())
    # REDQ's hidden 64 x 64 forward launches (test_gpu_redq.py counts them by hand): G (1 + M + E) + 1 + E
    nets = lambda step: npth.ens_nets("redq", step, 5, (64, 64), 7, (64, 64), 3, 2)
    got = npth.expected_engine_counts([nets("critic")] * 2 + [nets("policy")], True, 4096, 2)
    assert got[("k_gemm_fwd", 4096, 64, 64)] == {1: 2 * (1 + 2 + 3) + 1 + 3} and set(got[("k_gemm_fwd", 4096, 64, 7)]) == {0}


@pytest.mark.parametrize("algo,name", CASES, ids=IDS)
def test_a_float32_twin_uses_at_most_half_of_each_bar(algo, name):
    c = _case(algo, name)
    ex, new, met = _reference(algo, name)
    new32, met32 = c.twin(ex, np.float32)[:2]
    gap = c.figures(new32, ec.m_redq.twin_metrics_vector(met32), new, met)
    print(f"{algo} {name}: float32 twin against float64 twin: " + " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
    bad = {k: (v, ec.BARS[k]) for k, v in gap.items() if k not in ("pv", "qv") and not v <= 0.5 * ec.BARS[k]}
    assert not bad, bad
    # the second moments: float32's 1 - 0.999, as recorded; the rule max(bar, 2 gap) leaves every bar at its one-step value
    assert all(abs(gap[k] - ec.F32_GAP[algo][name][k]) < 1.5e-6 for k in ("pv", "qv")), (gap["pv"], gap["qv"])
    assert c.bars() == ec.BARS


# the figure each fault lands in, and what it cannot reach: the policy step runs after the critic steps, so a fault of its own leaves
# the critics' moments exact; TQC's policy loss reads the critics from before their step, so a critic-gradient fault leaves pm exact
LANDS_IN = {"tail_row": "qm", "last_column": "pm", "last_net": "qm"}


@pytest.mark.parametrize("what", ec.PERTURBATIONS)
@pytest.mark.parametrize("algo,name", CASES, ids=IDS)
def test_the_bars_see_tail_faults(algo, name, what):
    c = _case(algo, name)
    if what == "last_net" and c.E == 1:
        return
    ex, new, met = _reference(algo, name)
    with ec.perturbed(algo, what):
        bad, bad_met = c.twin(ex)[:2]
    again = c.twin(ex)[:2] if name == "narrow" else None             # the patch is gone afterwards
    assert again is None or all(np.array_equal(again[0][k], new[k]) for k in ec.m_redq.tw.STATE_KEYS)
    f, bars = c.figures(bad, ec.m_redq.twin_metrics_vector(bad_met), new, met), c.bars()
    ratio = {k: v / bars[k] for k, v in f.items()}
    print(f"{algo} {name} {what}: figure / bar " + " ".join(f"{k} {v:.3g}" for k, v in ratio.items() if v > 1))
    assert ratio[LANDS_IN[what]] > 10, ratio
    if what == "last_column":
        assert f["qm"] == 0 and f["qv"] == 0 and f["Qmax"] == 0               # the critics' state is out of this fault's reach
    if what == "tail_row" and algo == "tqc":
        assert f["pm"] == 0
