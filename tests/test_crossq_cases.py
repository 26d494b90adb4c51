"""CPU: the shape cases of test_gpu_crossq_shapes.py (tests/crossq_cases.py) and the large shapes of test_gpu_brn.py before any device
sees them.

  - every path the case table names is recomputed from the mirror of the host code (tests/net_paths.py, num_cus 256): cq_dw's
    bands, where cq_images' lists end, the engine of every GEMM shape, the column sums' rows per slab and the element-wise walk;
  - every case is usable() (test_gpu_crossq.py's conditions) and its float32 twin with double column sums is within half of each
    one-step bar of the float64 twin, so max(bar, 2 gap) is the one-step bar and a miss on the device is a kernel's, not the inputs';
  - the bars see a wrong tail: the float64 twin with the last row of the joint pass left out of the column sums, with the last
    action column of dQ/da zeroed, or with the last critic evaluated on its neighbour's parameters misses the bar of the quantity
    that fault lands in by more than a factor of ten;
  - test_gpu_brn.py's LARGE shapes reach the branches they are there for, and its statistics bar sees a dropped last slab."""
import functools

import numpy as np
import pytest

import crossq_cases as cc
import net_paths as npth
import test_gpu_brn as brn

NC = 256


@functools.lru_cache(maxsize=None)
def _case(name):
    return cc.shape_case(name, NC)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(mid, new, met, infos) of the float64 twin: computed once, read by every test of the case"""
    c = _case(name)
    return c.twin(c.state)


def _counts(c, updates, bx=True):
    return npth.cq_engine_counts(updates, bx, NC, c.O, c.ph, c.Oc + c.A, c.qh, c.E, c.B)


def _lists(c):
    return [npth.cq_image_list(u, c.O, c.ph, c.Oc + c.A, c.qh, c.E, c.B) for u in ("critic", "policy")]


def test_the_mirrors_of_crossq_and_brn():
    assert npth.choose_mc(24, 256, 256) == (32, 1) and npth.choose_mc(4098, 2, 256) == (64, 65) and npth.choose_mc(8192, 1, 256) == (32, 256)
    # 64 x 64 over 8192 rows: 256 slabs, the 64-outputs-a-workgroup reduction; one band
    assert npth.cq_dw_blocks(256, 8192, 64, 64) == 64 + 4 and npth.cq_dw_bands(256, 8192, 64, 64) == [64]
    assert npth.cq_dw_bands(256, 16, 2048, 2048) == [256] * 8                                  # test_gpu_crossq.py's `wide`: no ragged band
    assert [npth.brn_rows_per_slab(256, M) for M in (2, 8192, 65536, 65537, 65610, 2 ** 31 - 1)] == [64, 64, 64, 65, 65, 2097152]
    assert npth.brn_rows_per_slab(0, 100) == 64 and npth.brn_rows_per_slab(1, 257) == 65
    assert npth.brn_walk(8192, 64) == (131072, 1, 0, False)                                       # the largest product before LARGE
    # the lists of test_gpu_crossq.py's rows4096 and its counts by hand: 64 x 64 forwards E at 8192 rows, 2 + E at 4096
    got = npth.cq_engine_counts(("critic", "policy"), True, 256, 5, [64, 64], 7, [64, 64], 2, 4096)
    assert got[("k_gemm_fwd", 8192, 64, 64)] == {1: 2} and got[("k_gemm_fwd", 4096, 64, 64)] == {1: 4}
    assert got[("k_gemm_fwd", 8192, 64, 7)] == {0: 2} and got[("k_gemm_fwd", 4096, 64, 5)] == {0: 2} and got[("k_gemm_dx", 8192, 64, 64)] == {1: 2}
    assert got[("k_gemm_dx", 8192, 7, 64)] == {0: 2} and got[("k_gemm_dx", 4096, 7, 64)] == {0: 2} and got[("k_gemm_dw", 64, 64, 8192)] == {1: 2}


@pytest.mark.parametrize("name", cc.NAMES)
def test_shape_case_reaches_its_paths(name):
    """the case table's claims, from the host code's arithmetic"""
    c = _case(name)
    A, B, O, Oc, E, ph, qh = c.A, c.B, c.O, c.Oc, c.E, c.ph, c.qh
    cin, ldc = Oc + A, npth.pad4(Oc + A)
    lists = _lists(c)
    cuts = [npth.image_cut(l) for l in lists]
    jobs = [npth.trunk_images([n[:3] for n in l])[1] for l in lists]
    crit, pol = _counts(c, ("critic",)), _counts(c, ("policy",))
    engines = lambda counts, kernel=None: {e for k, v in counts.items() if kernel in (None, k[0]) for e in v}

    def act64():
        return A == 64 and npth.ens_sample_rows_per_block(A) == (4, 0) and 2 * A == 128 and c.asym and Oc == 29 and Oc % 4 != 0 and cin == 93 and \
            cin % 4 != 0 and B % 2 == 1 and 2 * B == npth.BRN_SLAB_ROWS + 10 and npth.brn_rows_per_slab(NC, 2 * B) == 64 and E == 3 and \
            len(ph) == len(qh) == 3 and engines(crit) | engines(pol) == {0}

    def wide_policy():
        up, down = npth.cq_dw_bands(NC, B, 1984, 2048), npth.cq_dw_bands(NC, B, 2048, 1984)
        return ph == [2048, 1984] and qh == [1984, 2048] and up == [256] * 7 + [192] and down == [512] * 4 and \
            npth.cq_dw_blocks(NC, B, 512, 1984) == 4092 <= npth.REDUCE_MAX_BLOCKS < npth.cq_dw_blocks(NC, B, 1024, 1984) and \
            npth.cq_dw_bands(NC, 2 * B, 1984, 2048) == up and ("k_gemm_dw", 192, 2048, 2 * B) in crit and ("k_gemm_dw", 512, 1984, B) in pol and \
            pol[("k_gemm_dw", 512, 1984, B)] == {0: 4} and crit[("k_gemm_dw", 256, 2048, 2 * B)] == {0: 7} and ph[-1] == 1984 and \
            c.h["adam_eps"] == 1e-5 and E == 1 and B < 64

    def half_split():
        hidden, first = ("k_gemm_fwd", 2 * B, 128, 256), ("k_gemm_fwd", 2 * B, 256, 62)
        at_b = {k: v for k, v in crit.items() if B in k[1:]}
        return 2 * B >= npth.SPLIT_ROWS > B and (2 * B) % 4 != 0 and len(lists[0]) == E and lists[1] == [] and cuts == [None, None] and \
            crit[hidden] == {1: E} and crit[first] == {0: E} and crit[("k_gemm_dx", 2 * B, 256, 128)] == {1: E} and \
            crit[("k_gemm_dx", 2 * B, 62, 256)] == {0: E} and crit[("k_gemm_dw", 62, 256, 2 * B)] == {1: E} and \
            crit[("k_gemm_dw", 256, 128, 2 * B)] == {1: E} and (O, cin) == (45, 62) and at_b and engines(at_b) == {0} and engines(pol) == {0}

    def e16_cut():
        both_c = {k for k, v in crit.items() if len(v) == 2}
        both_p = {k for k, v in pol.items() if len(v) == 2}
        return E == 16 and B >= npth.SPLIT_ROWS and cuts == [(1 + 5, 2), (1 + 5, 1)] and jobs == [3 + 5 * 5 + 1 + 2, 5 + 5 * 5 + 1] and \
            jobs[0] + 2 > npth.BX_MAX_JOBS and jobs[1] + 2 > npth.BX_MAX_JOBS and O % 4 == 0 and cin % 4 == 0 and c.asym and \
            ("k_gemm_fwd", 2 * B, 192, 128) in both_c and ("k_gemm_dx", 2 * B, 128, 192) in both_c and ("k_gemm_fwd", B, 128, 64) in both_p and \
            crit[("k_gemm_fwd", 2 * B, 192, 128)] == {1: 5, 0: 11} and pol[("k_gemm_fwd", B, 128, 64)] == {1: 1 + 5, 0: 11} and A == 3

    def many_rows():
        g0, steps0, cg0, carry0 = npth.brn_walk(2 * B, ldc)
        g1, steps1, cg1, carry1 = npth.brn_walk(2 * B, 64)
        return B == 128 * NC + 37 and 2 * B == 256 * NC + 74 and npth.brn_rows_per_slab(NC, 2 * B) == 65 and npth.brn_rows_per_slab(NC, B) == 64 and \
            (cin, ldc // 4) == (65, 17) and steps0 == 2 and carry0 and cg0 == 16 and steps1 == 2 and cg1 == 0 and not carry1 and \
            npth.elem_grid(g0)[1] and npth.elem_grid(g1)[1] and npth.div_up(B, 256) > 1 and A == 1 and E == 1 and cuts == [None, None]

    def ties():
        n, s = c.qs.n_params, c.qs.n_stats
        tied = cc.tied_rows(c, _reference(name)[0])
        return E == 3 and np.array_equal(c.state["qp"][2 * n:], c.state["qp"][:n]) and np.array_equal(c.state["qs"][2 * s:], c.state["qs"][:s]) and \
            not np.array_equal(c.state["qp"][n:2 * n], c.state["qp"][:n]) and 4 * int(tied.sum()) >= B

    ok = {"act64": act64, "wide_policy": wide_policy, "half_split": half_split, "e16_cut": e16_cut, "many_rows": many_rows, "ties": ties}[name]()
    assert ok, (name, cuts, jobs, sorted(crit.items()), sorted(pol.items()))
    assert (c.cbatch is not None) == c.asym and 1 <= E <= 16 and A <= 64 and 1 <= len(qh) <= 3 and max(ph + qh) <= 2048
    # without the split-operand engine: the same launches, all on the exact engine
    off = _counts(c, ("critic", "policy"), False)
    on = _counts(c, ("critic", "policy"))
    assert engines(off) == {0} and {k: sum(v.values()) for k, v in off.items()} == {k: sum(v.values()) for k, v in on.items()}


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_is_usable_and_its_float32_twin_uses_at_most_half_of_each_bar(name):
    c = _case(name)
    mid, new, met, infos = _reference(name)
    assert all(i["vmin"] >= cc.m.VAR_FLOOR and not i["warmed"] for i in infos), name                    # Case.usable(), from the cached twin
    ok, gap = cc.gap_ok(c, ref=(new, met))
    print(f"{name}: double-sum float32 twin against the float64 twin: " + " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
    assert ok, {k: (v, cc.BARS[k]) for k, v in gap.items() if not v <= 0.5 * cc.BARS[k]}


def test_e16_cut_has_no_unit_at_its_relu_kink():
    """what crossq_cases.E16_DENSE_BIAS is for: no hidden pre-activation of the critics' joint pass lies within 1e-6 of 0 -- ten times
    the distance (7.6e-8) at which the device was seen to take a derivative on the other side than the float64 twin.  With a bias of 0
    the same seed has such units (about 40 on every seed looked at)"""
    c = _case("e16_cut")
    assert c.h["adam_eps"] == 1e-5 and cc.table_row("e16_cut")[9] == cc.E16_DENSE_BIAS
    least = cc.min_preactivation(c, _reference("e16_cut")[3][0]["a2"])
    print(f"e16_cut: smallest |pre-activation| of the joint pass {least:.2e}")
    assert least >= 1e-6, least
    plain = cc.m.Case("e16_cut", cc.SEEDS["e16_cut"], cc.table_row("e16_cut")[:9] + (0.0,))
    assert cc.min_preactivation(plain) < 1e-6


LANDS_IN = cc.LANDS_IN


@pytest.mark.parametrize("what", cc.PERTURBATIONS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_the_bars_see_tail_faults(name, what):
    """Measured, figure / bar of the quantity the fault lands in: tail_row qm 1.7e4 (act64), 1.4e4 (wide_policy), 531 (half_split), 4.9e3
    (ties), 17 (many_rows: one row of 65610; its seed is chosen for it, crossq_cases.SEEDS) and, at e16_cut, what the run prints;
    last_column pm 238 to 9.0e3; last_net qm 3.3e4 to 8.1e4."""
    c = _case(name)
    if what == "last_net" and c.E == 1:
        return
    _, new, met, _ = _reference(name)
    with cc.perturbed(c, what):
        _, bad, bad_met, _ = c.twin(c.state)
    f = cc.m.figures(bad, cc.m.metrics_vector(bad_met), new, met)
    ratio = {k: v / cc.BARS[k] for k, v in f.items()}
    print(f"{name} {what}: figure / bar " + " ".join(f"{k} {v:.3g}" for k, v in ratio.items() if v > 1))
    assert max(ratio[k] for k in LANDS_IN[what]) > 10, ratio
    if what == "last_column":
        assert f["qm"] == 0 and f["qs"] == 0 and f["Qmax"] == 0                 # the critics' state is out of this fault's reach
    if name == "ties":                                                         # the patch is gone afterwards
        again = c.twin(c.state)[1]
        assert all(np.array_equal(again[k], new[k]) for k in cc.tw.STATE_KEYS)


def test_a_seed_of_minus_one_over_b_to_both_tied_critics_misses_the_bars():
    """what k_crossq_policy_seed's `ties` division is for: without it a tied row's dQ/da is doubled"""
    c = _case("ties")
    mid, new, met, _ = _reference("ties")
    tied = cc.tied_rows(c, mid)

    def wrap(backward):            # the policy update's critic seeds [B, 1]: -1 / (2 B) on a tied row of a tied critic, doubled to -1 / B
        def f(spec, caches, d_out, *a, **k):
            if spec is c.qs and d_out.shape == (c.B, 1):
                d_out = np.where(tied[:, None], 2 * d_out, d_out)
            return backward(spec, caches, d_out, *a, **k)
        return f
    with cc._patched("net_backward", wrap):
        _, bad, bad_met, _ = c.twin(c.state)
    f = cc.m.figures(bad, cc.m.metrics_vector(bad_met), new, met)
    assert f["pm"] > 10 * cc.BARS["pm"] and f["qm"] == 0, f


# ------------------------------------------------------------------------------------------- test_gpu_brn.py's LARGE shapes
def test_large_brn_shapes_reach_their_branches():
    shapes = [(brn.rows_of(M, NC), D, ld, E) for M, D, ld, E in brn.LARGE]
    assert [brn.reaches(M, ld, NC) for M, D, ld, E in shapes] == [(False, True), (True, True), (True, False), (True, False)]
    assert all(not any(brn.reaches(M, ld, NC)) for M, D, ld, E in brn.SHAPES)                          # and no older shape does
    M = shapes[0][0]
    assert npth.brn_rows_per_slab(NC, M) == 65 and M % 65 != 0                                          # the last slab is short
    assert npth.brn_walk(shapes[1][0], 64) == (1049616, 2, 0, False)                                    # just past the cap: step_cg 0
    groups, steps, step_cg, carries = npth.brn_walk(45000, 192)
    assert groups == 2160000 and steps == 3 and groups > 2 * 4096 * 256 and carries and 192 // 4 == 48  # two to three steps a thread
    assert npth.brn_walk(2100, 2048)[1] == 2 and all(E * M * ld * 4 <= 40e6 for M, D, ld, E in shapes)


def test_the_statistics_bar_sees_a_dropped_last_slab():
    """the twin with the rows of the last slab left out of the statistics (summed over the others, divided by M) misses STAT_BAR by
    more than ten times on the first LARGE shape"""
    M, D, ld, E = brn.rows_of(brn.LARGE[0][0], NC), *brn.LARGE[0][1:]
    c = brn.make_case(M, D, ld, E, si=len(brn.SHAPES))
    brn.check_margins(c)
    exp = brn.twin(c, "cold", False)
    keep = (M // npth.brn_rows_per_slab(NC, M)) * npth.brn_rows_per_slab(NC, M)
    assert 0 < M - keep < 65

    def wrap(stats):
        def f(x):
            mu = x[:keep].sum(axis=0) / M
            return mu, np.maximum(0, (x[:keep] * x[:keep]).sum(axis=0) / M - mu * mu)
        return f
    with cc._patched("brn_batch_stats", wrap):
        bad = brn.twin(c, "cold", False)
    miss = [brn._rel(bad["stats"][0, :D], exp["stats"][0, :D]), brn._rel(bad["stats"][0, D:], exp["stats"][0, D:])]
    print(f"dropped last slab of {M - keep} rows in {M}: mean {miss[0]:.2e} var {miss[1]:.2e} against {brn.STAT_BAR:.0e}")
    # the advanced variance misses by 77 times (the 16 rows of the far-off column are 2.4e-4 of its sum of squares); the advanced mean
    # by 2.3: it moves by (1 - momentum) 16 / M of itself
    assert miss[1] > 10 * brn.STAT_BAR and miss[0] > brn.STAT_BAR, miss
