"""CPU: the case table of test_gpu_ppo_lstm_shapes.py (tests/ppo_lstm_cases.py) and the mirrors it is built on (tests/net_paths.py:
lstm_check_desc, lstm_blocks, ppo_lstm_pass, lstm_act_fused): the mirror's flat layout against the library's and the oracle's, the
table's shapes against the restated clauses of check_lstm_desc, what the table covers, no case on a clip boundary, and -- the
condition the inputs are chosen under -- the same oracle evaluated in float32 within half of every bar the device is held to, so
that a miss on the device is the kernels' and not the inputs'."""
import numpy as np
import pytest

import net_paths as npth
import ppo_lstm_cases as lc
from rlx_amd.hip import lib as L
from rlx_amd.hip.lib import lstm_policy_desc


def _desc(O, A, E, H, torso, cell, combine, share=False):
    return lstm_policy_desc(O, A, E, H, torso, share, cell, combine)


@pytest.mark.parametrize("name", lc.NAMES)
def test_mirror_layout_matches_the_library_and_the_oracle(name):
    import ctypes
    c = lc.CASES[name]
    spec = lc.ol.LstmPolicySpec(c.O, c.A, c.E, npth.LSTM_H, c.torso, c.share, c.cell, c.combine)
    bl, n = npth.lstm_blocks(c.O, c.A, c.E, c.torso, c.share, c.cell == "gru", c.combine == "film")
    lib = L.load_library()
    d = _desc(*c.desc_args, share=c.share)
    assert int(lib.rlx_lstm_policy_param_count(ctypes.byref(d))) == n == spec.n_params
    assert [(k, o, ln) for k, (o, ln) in spec.off.items()] == bl


def test_accepted_cases_are_accepted_and_refused_ones_refused_for_the_stated_reason():
    for c in lc.CASES.values():
        assert npth.lstm_check_desc(*c.desc_args) is None, c.name
        assert 1 <= c.ne <= c.N and c.T >= 1
    for E in lc.ACT_E:
        for torso in lc.ACT_TORSO:
            for A in lc.ACT_A:
                for O in lc.ACT_O:
                    assert npth.lstm_check_desc(O, A, E, npth.LSTM_H, torso, 0, 0) is None
                    assert npth.lstm_act_fused(E, torso, A, False, O, (512, 256, 128))
    for what, (E, torso, A, combine) in lc.ACT_OUTSIDE.items():
        assert npth.lstm_check_desc(17, A, E, npth.LSTM_H, torso, 0, 1 if combine == "film" else 0) is None, what
        assert not npth.lstm_act_fused(E, torso, A, combine == "film", 17, (512, 256, 128)), what
    assert npth.lstm_act_fused(192, (512, 256, 128), 32, False, 23, (256, 128)) and not npth.lstm_act_fused(192, (512, 256, 128), 32, False, 23, (256, 132))
    ok = lc._refused()
    assert npth.lstm_check_desc(*ok) is None
    for name, args in lc.REFUSED.items():
        code, msg = npth.lstm_check_desc(*args)
        field = lc.REFUSED_FIELD[name.rsplit("_", 1)[0]]
        assert field in msg, (name, msg)
        assert code == (npth.RLX_EINVAL if field in ("cell", "combine") else npth.RLX_EUNSUP)
        # the one field the case changes is the reason: every other field is the accepted case's
        assert sum(a != b for a, b in zip(args, ok)) == 1, name
    # the clauses the issue lists, each with a case
    assert {"obs_0", "obs_33", "hidden_128", "enc_96", "enc_576", "torso0_96", "torso0_576", "torso1_6", "torso2_0", "act_0", "act_65",
            "cell_2", "combine_2", "torso0_0", "torso0_neg64", "torso1_0", "torso1_neg64"} <= set(lc.REFUSED)


def test_the_table_covers_what_it_is_meant_to():
    cs = list(lc.CASES.values())
    has = lambda f: any(f(c) for c in cs)
    branches = {
        "lstm": lambda c: c.cell == "lstm", "gru": lambda c: c.cell == "gru",
        "concat": lambda c: c.combine == "concat", "film": lambda c: c.combine == "film",
        "separate encoders": lambda c: not c.share, "shared encoder": lambda c: c.share,
        "full tiles only": lambda c: c.ne % npth.LSTM_ROWS == 0,
        "ragged last tile": lambda c: 1 < c.ne % npth.LSTM_ROWS,
        "a tile with a single env": lambda c: c.ne % npth.LSTM_ROWS == 1 and c.ne > npth.LSTM_ROWS,
        "a single env in all": lambda c: c.ne == 1,
        "T = 1": lambda c: c.T == 1, "odd T > 1": lambda c: c.T > 1 and c.T % 2 == 1, "even T": lambda c: c.T % 2 == 0,
        "share with E > D1, concat": lambda c: c.share and c.E > c.torso[0] and c.combine == "concat",
        "share with E > D1, film": lambda c: c.share and c.E > c.torso[0] and c.combine == "film",
        "every width at its minimum": lambda c: (c.O, c.A, c.E, c.torso) == (1, 1, 64, (64, 4, 4)),
        "O, A, E, torso[0] at their maximum": lambda c: (c.O, c.A, c.E, c.torso[0]) == (32, 64, 512, 512),
        "A > 8": lambda c: c.A > 8, "widths off the 64 grid": lambda c: c.torso[1] % 64 and c.torso[2] % 64,
        "env indices are a strict subset": lambda c: c.ne < c.N,
        "exactly 4096 rows": lambda c: c.T * c.ne == 4096, "4096 rows and a ragged tile": lambda c: c.T * c.ne > 4096 and c.ne % npth.LSTM_ROWS,
        "K1 = 128 on the split engine": lambda c: c.expect()["split"] and c.E + (0 if c.combine == "film" else 64) == 128,
        "K1 = 192 on the split engine": lambda c: c.expect()["split"] and c.E + (0 if c.combine == "film" else 64) == 192,
    }
    missing = [k for k, f in branches.items() if not has(f)]
    assert not missing, missing
    # the recurrent product: both engines on full and on ragged launches
    seen = {(lc.CASES[n].expect(o)["recurrent"], lc.CASES[n].expect(o)["full_tiles"]) for n, _, o in lc.RUNS if lc.CASES[n].cell == "lstm"}
    assert seen == {("split", True), ("split", False), ("exact", True), ("exact", False)}
    assert {l for _, l, _ in lc.RUNS} == {"defaults", "gemm_bx0", "bx_debug256"}
    # the engines: below 4096 rows nothing on the split engine; from there on everything but the FiLM pair
    for c in cs:
        rows = c.expect()["rows"]
        M = c.T * c.ne
        if M < 4096:
            assert all(k[1] == npth.ENGINE_EXACT for k in rows), c.name
        else:
            exact = {k for k in rows if k[1] == npth.ENGINE_EXACT}
            film = {("k_gemm_fwd", 0, M, 2 * c.E, 64), ("k_gemm_dx", 0, M, 64, 2 * c.E)} if c.combine == "film" else set()
            assert exact == film, (c.name, exact)
            assert not any(k[1] == npth.ENGINE_SPLIT for k in c.expect({"gemm_bx": 0})["rows"])
    assert set(lc.UPDATE_NAMES) <= set(lc.CASES) and lc.AFTER_REFUSAL in lc.CASES
    assert any(lc.CASES[n].cell == "gru" for n in lc.UPDATE_NAMES) and any(lc.CASES[n].O == 1 for n in lc.UPDATE_NAMES)


def _boundary_check(name, ratio):
    gap = np.abs(np.abs(ratio - 1.0) - lc.CLIP).min()
    assert gap > lc.RATIO_MARGIN, (name, gap)
    frac = (np.abs(ratio - 1.0) > lc.CLIP).mean()
    if ratio.size > 1:          # (one row: its clip fraction is 0 or 1 whatever the inputs)
        assert 0.0 < frac < 1.0, (name, frac)
    return gap, frac


@pytest.mark.parametrize("name", lc.NAMES)
def test_no_case_sits_on_a_clip_boundary(name):
    c = lc.case(name)
    met, _, _, ratio = c.oracle
    gap, frac = _boundary_check(name, ratio)
    assert frac == met["policy_ratio/clip_fraction"]
    print(name, f"closest ratio to 1 +- clip: {gap:.2e}; clip fraction {frac:.3f}")


@pytest.mark.parametrize("name", lc.NAMES)
def test_a_float32_evaluation_uses_at_most_half_of_each_bar(name):
    c = lc.case(name)
    met, gp, gc, _ = c.evaluate(np.float32)
    m = [met[k] for k, _, _ in lc.METRICS] + [met["policy_ratio/clip_fraction"]]
    rows, blocks, whole = lc.compare(c.spec, c.T, c.ne, c.oracle, m, gp, gc)
    print(name, "float32 on the CPU: ||dg||/||g||", {k: float(f"{v:.2e}") for k, v in whole.items()},
          "worst block, fraction of its bar:", max((max(b[0] / b[1], b[2] / b[3]), k) for k, b in blocks.items()))
    lc.assert_within(rows, blocks, whole, 0.5)


@pytest.mark.parametrize("name", lc.UPDATE_NAMES)
def test_float32_trajectory_leaves_no_parameter_outside_the_update_bar(name):
    """four updates from opt_count = 3 with clipping active: gradients by float32 autograd against float64 autograd (float32 optimizer
    state on both sides, as on the device)"""
    u = lc.UPDATES[name].build()
    o64, p64, c64 = u.trajectory64
    o32, p32, c32 = u.trajectory(np.float32)
    assert u.n_upd == 4 == len(o64) and u.idx.shape == (4, u.ne) and u.N == 2 * u.ne
    g = u.max_grad_norm
    assert o64[0]["gradients/policy_grad_norm"] > g and o64[0]["gradients/critic_grad_norm"] > g          # clipping acts
    for i in range(u.n_upd):      # no update's minibatch on a clip boundary either
        _boundary_check((name, i), lc.loss_and_grads(u.spec, u.p, u.cs, u.cp, u.rollout, u.idx[i], np.float64)[3])
    for a, b in zip(o32, o64):
        for k in b:
            if k != "policy_ratio/clip_fraction":
                assert abs(a[k] - b[k]) <= 0.5 * (2e-5 + 2e-3 * abs(b[k])), (k, a[k], b[k])
    for got, exp, start in ((p32, p64, u.p), (c32, c64, u.cp)):
        d = np.abs(got.astype(np.float64) - exp)
        print(name, f"float32 trajectory: max |dp| {d.max():.2e}")
        assert (d <= 2e-5 + 1e-3 * np.abs(exp)).all()          # the float32 reference alone leaves out nothing (the device may: 0.001)
        assert np.abs(exp.astype(np.float64) - start).max() > 1e-4
