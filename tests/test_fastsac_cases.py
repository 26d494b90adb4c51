"""CPU: the FastSAC oracle (oracle/fastsac.py) at hidden widths other than the reference's -- its flat layout against the library's
(rlx_lnmlp_param_count) -- and the shape cases of test_gpu_fastsac_shapes.py: every state vector moves in both updates, clipping
acts where a case switches it on, and the split-engine cases' operands sit inside the fp16 window (gemm_bx.h)."""
import numpy as np
import pytest

import fastsac_cases as fc
from net_paths import F16_MAX, X_ALIMIT, X_WLIMIT
from oracle import fastsac as ofs
from rlx_amd.hip import lib as L
from rlx_amd.hip import lnmlp_desc


@pytest.mark.parametrize("in_dim,hidden,out_dim", [(94, (128, 64, 64, 64), 65), (5, (64,), 2), (72, (768, 192), 51), (33, (704, 64), 130)])
def test_flat_layout_matches_the_library(in_dim, hidden, out_dim):
    import ctypes
    n = ofs.param_count(in_dim, hidden, out_dim)
    d = lnmlp_desc(in_dim, hidden, out_dim)
    assert int(L.load_library().rlx_lnmlp_param_count(ctypes.byref(d))) == n
    bl = ofs.blocks(in_dim, hidden, out_dim)
    assert bl[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(bl, bl[1:])) and bl[-1][1] + bl[-1][2] == n
    widths = [in_dim] + list(hidden)
    want = [x for l, w in enumerate(hidden) for x in (("W%d" % l, widths[l] * w), ("b%d" % l, w), ("g%d" % l, w), ("be%d" % l, w))]
    want += [("Wh", hidden[-1] * out_dim), ("bh", out_dim)]
    assert [(name, size) for name, _, size in bl] == want
    # make_params lays its networks out the same way: the LayerNorm scales sit near 1 exactly in the g blocks
    p, q = ofs.make_params(3, in_dim, 1, out_dim, in_dim - 1, policy_hidden=hidden, critic_hidden=hidden)
    assert q[0].size == n and p.size == ofs.param_count(in_dim, hidden, 2)
    for name, off, size in bl:
        assert (abs(q[0][off:off + size].mean() - 1.0) < 0.1) == name.startswith("g"), name


def test_default_widths_are_the_default():
    a = ofs.make_params(5, 7, 2, 21)
    b = ofs.make_params(5, 7, 2, 21, None, ofs.POLICY_HIDDEN, ofs.CRITIC_HIDDEN)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("name", ["narrow", "act65", "dxlds"])
def test_small_cases_move_every_vector_in_both_steps(name):
    c = fc.shape_case(name)
    st1, cmet, pmet, (rc, rp) = c.twin(c.state, c.noise(), 1)
    assert all(np.all(np.isfinite(np.asarray(v))) for v in st1.values()) and np.all(np.isfinite(cmet)) and np.all(np.isfinite(pmet))
    for k in ("P", "Q", "QT", "la"):
        assert np.any(np.asarray(st1[k]) != np.asarray(c.state[k])), k
    if c.h["max_grad_norm"] > 0:        # clipping acts in both updates
        assert cmet[5] > c.h["max_grad_norm"] and pmet[2] > c.h["max_grad_norm"]
    st1 = {k: fc._f32(v) if np.ndim(v) else float(np.float32(v)) for k, v in st1.items()}
    st2, cmet2, _, _ = c.twin(st1, c.noise(), 2)
    # the second step starts from non-zero moments and moves everything again
    assert all(np.any(st1[k] != 0) for k in ("pm", "pv", "qm", "qv")) and st1["am"] != 0
    assert all(np.any(st2[k] != st1[k]) for k in ("P", "pm", "pv", "Q", "qm", "qv", "QT"))
    assert st2["av"] > st1["av"] > 0 and st2["la"] != st1["la"]
    if name == "narrow":                # the one row's reward lies past v_max
        assert c.batch[3][0] > c.h["v_max"] and c.B == 1


@pytest.mark.parametrize("name", ["split4", "split_ragged"])
def test_split_engine_cases_stay_inside_the_fp16_window(name):
    """headroom of the operands the split engine turns into fp16 planes, from the oracle: weights below 1023 by > 100x, activations
    below 4094 by > 100x, scaled per-sample gradients below 65504 by > 10x (a NaN cannot come from the inputs)"""
    c = fc.shape_case(name)
    w = fc.fp16_window(c, c.state, c.noise(), 1)
    assert w["weight"] * 100 < X_WLIMIT and w["act"] * 100 < X_ALIMIT and 0 < w["grad_scaled"] * 10 < F16_MAX, w


@pytest.mark.parametrize("name", fc.NAMES)
def test_a_float32_evaluation_uses_at_most_half_of_each_bar(name):
    """the condition the cases' inputs are chosen under (fastsac_cases.HP): a plain float32 evaluation of the critic update -- the
    one with the categorical projection, the largest float32 error of either update -- is within half of the gradient bar (1e-5)
    and half of the parameter bar (1e-6) of the float64 oracle, so that a miss on the device is the kernels' and not the inputs'"""
    c = fc.shape_case(name)
    eps = c.noise()
    new, _, _, (rc, _) = c.twin(c.state, eps, 1)
    gq, _ = ofs.clip_grad_norm(np.concatenate([rc["g_q1"], rc["g_q2"]]), c.h["max_grad_norm"])
    g32, q32 = fc.float32_critic_update(c, c.state, eps)
    print(f"{name}: float32 on the CPU: critic gradient {fc._rel(g32, gq):.2e}, critics after the step {fc._rel(q32, new['Q']):.2e}")
    assert fc._rel(g32, gq) < 0.5e-5 and fc._rel(q32, new["Q"]) < 0.5e-6


def test_param_count_refuses_bad_layer_counts():
    import ctypes
    lib = L.load_library()
    for hidden in ((), (64,) * 5):
        d = lnmlp_desc(8, hidden, 4)
        assert lib.rlx_lnmlp_param_count(ctypes.byref(d)) == -1
    assert lib.rlx_lnmlp_param_count(None) == -1


@pytest.mark.parametrize("name", fc.NAMES)
def test_the_bars_see_weight_decay(name):
    """an update without AdamW's (1 - lr wd) factor -- the oracle with weight_decay 0 -- misses the 1e-6 bars on the policy, the
    critics, the targets' source and log_alpha in both steps: lr wd = 1.5e-5 is fifteen times the bar (fastsac_cases.HP)"""
    c = fc.shape_case(name)
    eps1, eps2 = c.noise(), c.noise()
    st = c.state
    for step, eps in ((1, eps1), (2, eps2)):
        new = c.twin(st, eps, step)[0]
        h = c.h
        c.h = dict(h, weight_decay=0.0)
        try:
            without = c.twin(st, eps, step)[0]
        finally:
            c.h = h
        for k in ("P", "Q"):
            assert fc._rel(without[k], new[k]) > 5e-6, (k, step, fc._rel(without[k], new[k]))
        assert fc._rel(without["QT"], new["QT"]) > 1e-6, (step, fc._rel(without["QT"], new["QT"]))
        assert abs(without["la"] - new["la"]) > 5e-6 * abs(new["la"])
        st = {k: fc._f32(v) if np.ndim(v) else float(np.float32(v)) for k, v in new.items()}
