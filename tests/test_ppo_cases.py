"""CPU: the case table of test_gpu_ppo_shapes.py (tests/ppo_cases.py) and the selection mirror it is built on (tests/net_paths.py:
ppo_pass): the mirror's flat layout against the library's, a case on each side of every predicate the host code branches on, every
case's inputs inside the fp16 window of the split operands, and -- the condition the inputs are chosen under -- a plain float32
evaluation of the oracle within half of every bar the device is held to, so that a miss on the device is the kernels' and not the
inputs'."""
import ctypes

import numpy as np
import pytest

import net_paths as npth
import ppo_cases as pc
from oracle import nets, prng
from rlx_amd.hip import lib as L
from rlx_amd.hip import mlp_desc


@pytest.mark.parametrize("name", pc.NAMES)
def test_mirror_layout_matches_the_library_and_the_oracle(name):
    c = pc.CASES[name]
    lib = L.load_library()
    for spec, out, logstd in ((c.ps, c.A, True), (c.cs, 1, False)):
        bl, n = npth.mlp_blocks(c.O, c.hidden, out, c.ln, logstd)
        d = mlp_desc(c.O, c.hidden, out, c.act, c.ln, logstd)
        assert int(lib.rlx_mlp_param_count(ctypes.byref(d))) == n == spec.n_params
        assert bl == pc.blocks(spec)
        assert bl[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(bl, bl[1:])) and bl[-1][1] + bl[-1][2] == n


def _passes():
    """(case, label, mirror result) of every run of the GPU test"""
    return [(c, label, c.expect(mo)) for c in pc.CASES.values() for label, _, mo in c.settings()]


def test_every_predicate_has_a_case_on_each_side():
    runs = _passes()
    nets_ = [(c, label, e, e[which], which) for c, label, e in runs for which in ("policy", "critic")]
    kernels = lambda e: {k[0] for k in e["rows"]}
    eng = lambda e, kernel: {k[1] for k in e["rows"] if k[0] == kernel}
    branches = {
        # tail_shape_ok / tail_rows
        "no tail": lambda c, l, e, p, w: p["tail"] == 0,
        "32-row tail": lambda c, l, e, p, w: p["tail"] == 32,
        "64-row tail, H2 256 wide, chosen by size": lambda c, l, e, p, w: p["tail"] == 64 and c.hidden[1] == 256 and c.act == nets.ACT_ELU,
        "64-row tail, H2 512 wide": lambda c, l, e, p, w: p["tail"] == 64 and c.hidden[1] == 512,
        "64-row tail, H2 384 wide": lambda c, l, e, p, w: p["tail"] == 64 and c.hidden[1] == 384,
        "64-row tail, H2 128 wide": lambda c, l, e, p, w: p["tail"] == 64 and c.hidden[1] == 128,
        "k_tail_bx<TANH>": lambda c, l, e, p, w: p["tail"] == 64 and c.act == nets.ACT_TANH,
        "k_tail_bx<RELU>": lambda c, l, e, p, w: p["tail"] == 64 and c.act == nets.ACT_RELU,
        "no tail: rows % 64": lambda c, l, e, p, w: p["tail"] == 0 and c.mb % 64 and c.mb % 32 == 0 and c.hidden[1:] == (256, 128) and c.A <= 8,
        "no tail: last width": lambda c, l, e, p, w: p["tail"] == 0 and len(c.hidden) == 3 and c.hidden[2] != 128,
        "no tail: H2 % 128": lambda c, l, e, p, w: p["tail"] == 0 and len(c.hidden) == 3 and c.hidden[2] == 128 and c.hidden[1] % 128,
        "no tail: H2 > 512": lambda c, l, e, p, w: p["tail"] == 0 and len(c.hidden) == 3 and c.hidden[2] == 128 and c.hidden[1] % 128 == 0 and c.hidden[1] > 512,
        "no tail: two hidden layers": lambda c, l, e, p, w: p["tail"] == 0 and len(c.hidden) == 2,
        "policy without the tail, critic with it": lambda c, l, e, p, w: w == "policy" and p["tail"] == 0 and e["critic"]["tail"] > 0,
        "A at the tail's limit": lambda c, l, e, p, w: w == "policy" and p["tail"] and c.A == 8,
        "A = 1 in the padded head": lambda c, l, e, p, w: w == "policy" and p["tail"] and c.A == 1,
        # twin_shapes_ok / twin_images
        "twin pass": lambda c, l, e, p, w: e["twin"],
        "twin forced but inadmissible": lambda c, l, e, p, w: l == "twin1" and not e["twin_ok"],
        "twin admissible, images missing": lambda c, l, e, p, w: l == "twin1" and e["twin_ok"] and not e["twin"],
        "twin inadmissible: last width": lambda c, l, e, p, w: not e["twin_ok"] and c.hidden[-1] not in (64, 128, 256) and c.act == nets.ACT_ELU,
        "twin inadmissible: A > 8": lambda c, l, e, p, w: not e["twin_ok"] and c.A > 8 and c.O <= 32,
        "twin inadmissible: first layer": lambda c, l, e, p, w: not e["twin_ok"] and c.act != nets.ACT_ELU,
        "twin with two hidden layers": lambda c, l, e, p, w: e["twin"] and len(c.hidden) == 2,
        "twin without the tail, three layers": lambda c, l, e, p, w: e["twin"] and len(c.hidden) == 3 and p["tail"] == 0,
        "twin with k_l1fwd_mfma": lambda c, l, e, p, w: e["twin"] and p["first"] == "l1fwd_mfma",
        # first layer forward
        "k_l12fwd, N2 256": lambda c, l, e, p, w: p["first"] == "l12fwd" and c.hidden[1] == 256,
        "k_l12fwd, N2 512": lambda c, l, e, p, w: p["first"] == "l12fwd" and c.hidden[1] == 512,
        "k_l12fwd, ragged last tile": lambda c, l, e, p, w: p["first"] == "l12fwd" and c.mb % 32,
        "k_l12fwd, h1 stored": lambda c, l, e, p, w: p["first"] == "l12fwd" and p["h1_stored"],
        "k_l12fwd, h1 recomputed": lambda c, l, e, p, w: p["first"] == "l12fwd" and not p["h1_stored"],
        "k_l1fwd_mfma + GEMM": lambda c, l, e, p, w: p["first"] == "l1fwd_mfma",
        "k_l1fwd_mfma: 9 k-steps": lambda c, l, e, p, w: p["first"] == "l1fwd_mfma" and c.O <= 18,
        "k_l1: no MFMA first layer": lambda c, l, e, p, w: p["first"] == "l1",
        "wide GEMM first layer": lambda c, l, e, p, w: p["first"] == "wide",
        "wide LayerNorm first layer": lambda c, l, e, p, w: p["first"] == "wide_ln",
        "wide rows re-pitched, records of 64 floats": lambda c, l, e, p, w: c.name in pc.UPDATE_NAMES and npth.row_pitch(c.O) != c.O and 32 < c.O + c.A + 3 <= 64,
        "wide rows re-pitched, records of 128 floats": lambda c, l, e, p, w: c.name in pc.UPDATE_NAMES and npth.row_pitch(c.O) != c.O and 64 < c.O + c.A + 3 <= 128,
        "wide rows re-pitched": lambda c, l, e, p, w: c.O > 32 and npth.row_pitch(c.O) != c.O,
        "wide rows at their own stride": lambda c, l, e, p, w: c.O > 32 and npth.row_pitch(c.O) == c.O,
        "observation operand: O = 1": lambda c, l, e, p, w: c.O == 1,
        "observation operand: O = 32": lambda c, l, e, p, w: c.O == 32,
        "observation operand: odd O": lambda c, l, e, p, w: c.O % 2 == 1 and 1 < c.O <= 32,
        # first layer backward
        "fused 512-ELU-LN first-layer backward": lambda c, l, e, p, w: p["l1bwd"] == "fused" and c.hidden[0] == 512,
        "fused 256-tanh first-layer backward": lambda c, l, e, p, w: p["l1bwd"] == "fused" and c.act == nets.ACT_TANH,
        "fused 256-ReLU first-layer backward": lambda c, l, e, p, w: p["l1bwd"] == "fused" and c.act == nets.ACT_RELU,
        "fused, without its split images": lambda c, l, e, p, w: p["l1bwd"] == "fused" and not p["l1bwd_split"] and eng(e, "k_dx_l1bwd") == {0},
        "unfused narrow first layer": lambda c, l, e, p, w: p["l1bwd"] == "unfused" and c.O <= 32 and len(c.hidden) >= 2,
        "unfused: one hidden layer": lambda c, l, e, p, w: len(c.hidden) == 1 and not c.ln,
        "unfused: one hidden layer under LayerNorm": lambda c, l, e, p, w: len(c.hidden) == 1 and c.ln and p["first"] == "l1fwd_mfma",
        "unfused: hidden[1] > 512 under the 512-ELU-LayerNorm first layer": lambda c, l, e, p, w: p["l1bwd"] == "unfused" and c.hidden[0] == 512 and len(c.hidden) == 3 and c.O <= 32,
        "unfused: hidden[0] % 128": lambda c, l, e, p, w: p["l1bwd"] == "unfused" and c.hidden[0] % 128 == 64 and c.hidden[0] > 64,
        # weight gradients
        "merged two-job weight gradient": lambda c, l, e, p, w: p["dw"] == "merged",
        "merged, N2 = 512, recomputed h1": lambda c, l, e, p, w: p["dw"] == "merged" and c.hidden[1] == 512 and not p["h1_stored"],
        "merged, stored h1": lambda c, l, e, p, w: p["dw"] == "merged" and p["h1_stored"],
        "separate weight gradients": lambda c, l, e, p, w: p["dw"] == "separate",
        "merge2 (wide, no LayerNorm)": lambda c, l, e, p, w: p["dw"] == "merge2",
        "wide first-layer weight gradient on the split engine": lambda c, l, e, p, w: ("k_gemm_dw", 1, c.O, c.hidden[0], c.mb) in e["rows"],
        "layer-3 input gradient as its own launch": lambda c, l, e, p, w: ("k_gemm_dx", 1, c.mb, c.hidden[1], c.hidden[-1]) in e["rows"] and len(c.hidden) == 3,
        # head
        "fast head K = 64": lambda c, l, e, p, w: p["head"] == "fast64",
        "fast head K = 128": lambda c, l, e, p, w: p["head"] == "fast128",
        "fast head K = 256": lambda c, l, e, p, w: p["head"] == "fast256",
        "generic head: K": lambda c, l, e, p, w: p["head"] == "generic" and c.hidden[-1] not in (64, 128, 256),
        "generic head: A > 8": lambda c, l, e, p, w: w == "policy" and p["head"] == "generic" and c.A > 8 and c.hidden[-1] == 128,
        "generic head, K = 512": lambda c, l, e, p, w: p["head"] == "generic" and c.hidden[-1] == 512,
        "head inside the tail": lambda c, l, e, p, w: p["head"] == "tail",
        "ragged rows in the head": lambda c, l, e, p, w: p["head"] != "tail" and c.mb % 64,
        # rows
        "rows % 128 != 0 in the 128-row GEMM tiles": lambda c, l, e, p, w: c.mb % 128 and c.mb % 64 == 0,
        "odd row count": lambda c, l, e, p, w: c.mb % 2 == 1,
        "default options": lambda c, l, e, p, w: l == "defaults" and 8192 < c.mb <= 16384,
    }
    # (bx_dw_usable has no false side here: from 4096 rows on, with the split engine on, it turns down only a width or a stride that is
    #  no multiple of 4 -- mlp_check_desc refuses such hidden widths and row_pitch pads such strides; below 4096 rows: test_gpu_mlp.py)
    missing = [name for name, f in branches.items() if not any(f(*x) for x in nets_)]
    assert not missing, missing
    # every kernel kind of the pass's profiler rows is predicted somewhere, on the engines the code can put it on
    seen = {(k[0], k[1]) for _, _, e in runs for k in e["rows"]}
    assert seen == {("k_gemm_fwd", 0), ("k_gemm_fwd", 1), ("k_gemm_dx", 1), ("k_gemm_dw", 1), ("k_dx_l1bwd", 0), ("k_dx_l1bwd", 1),
                    ("k_l1fwd_mfma", 2), ("k_head_loss", 2), ("k_reduce_segments", 2), ("k_l12fwd", 1), ("k_tail", 1)}, sorted(seen)
    # an engine-0 GEMM only where the code has no image to offer: a wide first layer's forward
    for c, _, e in runs:
        assert all(k[4] == c.O and c.O > 32 for k in e["rows"] if k[0] == "k_gemm_fwd" and k[1] == 0)
    # the twin schedule of the whole-update entry between 6144 and 16384 rows only
    assert npth.twin_default(*pc.CASES["mid"].shape) and not npth.twin_default(*pc.CASES["h2_512"].shape)
    assert not npth.twin_default(17, (512, 256, 128), 6, nets.ACT_ELU, True, 32768)


def test_the_bench_shape_is_what_test_gpu_bench_shapes_asserts():
    """the mirror at the one shape the suite held to the oracle before: the rows test_gpu_bench_shapes.py writes out by hand"""
    for MB, twin, tail, l12 in ((32768, 0, 1, 1), (32768, 0, 0, 0), (32768, 0, 1, 0), (4096, 1, 1, 1), (4096, 1, 0, 0), (4096, 1, 2, 1)):
        e = npth.ppo_pass(17, (512, 256, 128), 6, nets.ACT_ELU, True, MB, dict(ppo_twin=twin, ppo_tail=tail, l12_fused=l12))
        n = 1 if twin else 2
        l3 = (("k_tail", 1, MB, 128, 256),) if tail else (("k_gemm_fwd", 1, MB, 128, 256), ("k_gemm_dx", 1, MB, 256, 128))
        l2 = (("k_l12fwd", 1, MB, 256, 512),) if l12 else (("k_gemm_fwd", 1, MB, 256, 512),)
        dw = (("k_gemm_dw", 1, 768, 384, MB),) if tail else (("k_gemm_dw", 1, 256, 128, MB), ("k_gemm_dw", 1, 512, 256, MB))
        for key in (("k_dx_l1bwd", 1, MB, 512, 256),) + dw + l2 + l3:
            assert e["rows"].get(key) == n, (key, e["rows"])
        assert e["twin"] == bool(twin) and not any(k[1] == 0 for k in e["rows"])
        assert e["policy"]["tail"] == (0 if not tail else 64 if tail == 1 else 32)


@pytest.mark.parametrize("name", sorted(pc.REFUSED))
def test_refused_shapes_are_refused_by_the_mirror(name):
    code, msg = npth.ppo_refusal(*pc.REFUSED[name])
    assert code == -4 and msg
    assert all(npth.ppo_refusal(*c.shape) is None for c in pc.CASES.values())
    # what the pass answered before it gathered wide rows at a padded stride
    assert npth.ppo_refusal(*pc.CASES["wide33"].shape, repitch=False) == (-4, "mlp: wide inputs need a row stride that is a multiple of 4")
    assert npth.ppo_refusal(*pc.CASES["wide376"].shape, repitch=False) is None


def test_relu_case_gathers_no_row_with_a_unit_at_its_kink():
    c = pc.case("tail_relu")
    B = 2 * c.mb
    assert 0 < len(c.kinks) and B - c.pool.size <= len(c.kinks) and c.pool.size > 0.98 * B      # well under 2 % of the pool rejected
    assert len(set(c.idx.tolist())) == c.mb
    for spec, par in ((c.ps, c.pp), (c.cs, c.cp)):
        assert pc.kink_entries(spec, par.astype(np.float64), c.states[c.idx], pc.KINK) == []


@pytest.mark.parametrize("name", pc.NAMES)
def test_operands_lie_inside_the_fp16_window(name):
    c = pc.case(name)
    w = pc.fp16_window(c)
    print(name, {k: float(f"{v:.3g}") for k, v in w.items()})
    assert w["weight"] < npth.X_WLIMIT and w["act"] < npth.X_ALIMIT and 0 < w["grad_scaled"] < npth.F16_MAX, w
    assert len(set(c.idx.tolist())) == c.mb and c.idx.max() < 2 * c.mb


@pytest.mark.parametrize("name", pc.NAMES)
def test_a_float32_evaluation_uses_at_most_half_of_each_bar(name):
    c = pc.case(name)
    loss, met, gp, gc = c.evaluate(np.float32)
    m = [met[n] for n, _, _ in pc.METRICS] + [met["policy_ratio/clip_fraction"]]
    m[0], m[1], m[2] = (np.float64(x) for x in m[:3])
    rows, report = pc.compare(c, np.array(m, np.float64), gp, gc)
    rows["loss"] = (float(loss), rows["loss"][1], rows["loss"][2])
    print(name, "float32 on the CPU:", {k: float(f"{v:.2e}") for k, v in report.items()})
    for k, (got, exp, allowed) in rows.items():
        assert abs(got - exp) <= 0.5 * allowed, (k, got, exp, allowed)
    for k, v in report.items():
        assert v < 0.5 * pc.GRAD_BAR, (k, v)


@pytest.mark.parametrize("name", pc.UPDATE_NAMES)
def test_float32_trajectory_meets_the_update_bars_ten_times_over(name):
    """four updates of mb rows (T = 2, N = mb, two epochs) with clipping active: the float32 numpy update against the float64 one,
    held to a tenth of what test_gpu_ppo_shapes.py allows the device"""
    c = pc.case(name)
    o64, k64, p64, c64, n64 = c.update64
    o32, k32, p32, c32, n32 = c.update(np.float32, prng.prng_key(5))
    n_upd = 2 * pc.UPD_EPOCHS
    assert n64 == n32 == n_upd == len(o64) and np.array_equal(k64, k32)
    g = c.max_grad_norm
    assert all(o["gradients/policy_grad_norm"] > g and o["gradients/critic_grad_norm"] > g for o in o64[:1])      # clipping acts
    worst = 0.0
    for a, b in zip(o32, o64):
        for k in ("loss/policy_gradient_loss", "loss/critic_loss", "loss/entropy_loss", "policy_ratio/approx_kl", "gradients/policy_grad_norm",
                  "gradients/critic_grad_norm"):
            assert abs(float(a[k]) - float(b[k])) <= 0.1 * (2e-5 + 2e-3 * abs(float(b[k]))), (k, a[k], b[k])
            worst = max(worst, abs(float(a[k]) - float(b[k])) / max(abs(float(b[k])), 1e-3))
    for got, exp, start in ((p32, p64, c.pp), (c32, c64, c.cp)):
        d = np.abs(got.astype(np.float64) - exp)
        print(name, f"float32 trajectory: max |dp| {d.max():.2e}, metrics within {worst:.1e} relative")
        assert (d <= 2e-5 + 1e-3 * np.abs(exp)).all()          # the float32 reference alone leaves out nothing (the device may: 0.001)
        assert d.max() <= 0.1 * 2 * pc.LR * n_upd
        assert np.abs(exp - start).max() > 1e-4
