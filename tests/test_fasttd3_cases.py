"""CPU: the shape cases of test_gpu_fasttd3_shapes.py (tests/fasttd3_cases.py) before they meet the device.  The 1e-5 gradient
bar of FastTD3 is defined away from ReLU kinks and ties, with at most MAX_FLIPS candidates explained per update step: that cap is
a condition on the cases, so a plain float32 evaluation of each case (torch on the CPU) has to meet the bar within it.  The
split-engine cases' operands sit inside the fp16 window (gemm_bx.h): ReLU activations are not bounded by a norm."""
import numpy as np
import pytest

import fasttd3_cases as fc
import fasttd3_twin as tw
from net_paths import F16_MAX, X_ALIMIT, X_WLIMIT


@pytest.mark.parametrize("name", fc.NAMES)
def test_a_float32_evaluation_meets_the_bar_within_the_flip_cap(name):
    c = fc.shape_case(name)
    eps = c.noise()
    rc, rp = c.steps(c.state, eps)
    (gq, tq, cq, r0q), (gp, tp, cp, r0p) = fc.float32_flips(c, c.state, eps)
    print(f"{name}: float32 on the CPU: critic {r0q:.2e} with {len(tq)} of {len(cq)} candidates flipped, policy {r0p:.2e} with {len(tp)} of {len(cp)}")
    assert len(tq) <= fc.MAX_FLIPS and len(tp) <= fc.MAX_FLIPS
    rc32, rp32 = c.steps(c.state, eps, dtype=np.float32)
    g64 = lambda x: np.asarray(x, np.float64)
    assert fc._rel(g64(np.concatenate([rc32["g_q1"], rc32["g_q2"]])), gq) < 1e-5 and fc._rel(g64(rp32["g_policy"]), gp) < 1e-5
    if c.B <= 333 and name != "wide":       # the small cases: no candidate inside KINK_TAU at all (wide: 333 rows x 2048 units per critic)
        assert not cq and not cp, (cq, cp)
    if c.h["max_grad_norm"] > 0:            # clipping acts in both updates
        _, cmet, pmet = c.apply(c.state, 1, rc, rp)
        assert cmet[3] > c.h["max_grad_norm"] and pmet[1] > c.h["max_grad_norm"]


@pytest.mark.parametrize("name", ["split3", "split_ragged", "many_rows"])
def test_split_engine_cases_stay_inside_the_fp16_window(name):
    """headroom of the operands the split engine turns into fp16 planes, from the twin: weights below 1023 and activations below
    4094 by > 50x, scaled per-sample gradients below 65504 by > 10x (a NaN cannot come from the inputs)"""
    c = fc.shape_case(name)
    w = fc.fp16_window(c, c.state, c.noise())
    print(name, w)
    assert w["weight"] * 50 < X_WLIMIT and w["act"] * 50 < X_ALIMIT and 0 < w["grad_scaled"] * 10 < F16_MAX, w


def test_flat_layout_matches_the_twin():
    for in_dim, hidden, out in ((93, (128, 64, 64), 65), (5, (64,), 2), (64, (1024, 1024), 128)):
        bl = fc._blocks(in_dim, hidden, out)
        assert bl[-1][1] + bl[-1][2] == tw.param_count(in_dim, hidden, out)
        assert all(a[1] + a[2] == b[1] for a, b in zip(bl, bl[1:]))
