"""GPU: rlx_aqe_update_f32 -- the whole AQE update, G critic steps and one policy step -- against the float64 twin
(tests/aqe_twin.py) on the same float32 inputs, with the noise injected through rlx_dbg_set_sac_noise.

Inputs: tests/test_gpu_redq.py's recipe (tw.problem).  Figures (figures()) and their bars for ONE critic step (BARS) are
tests/test_gpu_redq.py's, restated as numbers: metrics 1e-5 relative and absolute, the two norms 1e-5 relative; first moments (a
first step's are gradients / 10) 1e-5 relative L2; second moments 5e-5 relative L2 (float32's 1 - 0.999 is 1.29e-5 off 0.001, in
every float32 Adam); parameter steps within 2e-5 on 99 % of the entries and within 2 lr + 1e-6 everywhere; log_alpha 1e-6; targets
rtol 1e-4, atol 2 lr tau + 1e-6.

Several critic steps, and 4096 rows, compound float32 rounding: the twin evaluated in numpy float32 on the same inputs is itself off
the float64 twin by F32_GAP below (measured once on a CPU: this file run as a script, repository root and rl-x_amd on PYTHONPATH).
Those cases are held to twice that gap or to the one-step bar, whichever is larger."""
import numpy as np
import pytest
import torch

import aqe_twin as tw
from oracle import nets, prng
from rlx_amd.hip import RlxError, mlp_desc

pytestmark = pytest.mark.gpu

GAMMA, TAU, LR = 0.99, 0.005, 3e-4
NAMES = tw.METRICS
KEY = prng.prng_key(11)

BARS = {"metrics": 1e-5, "norms": 1e-5, "pm": 1e-5, "qm": 1e-5, "pv": 5e-5, "qv": 5e-5, "la": 1e-6, "P99": 2e-5, "Q99": 2e-5,
        "Pmax": 2 * LR + 1e-6, "Qmax": 2 * LR + 1e-6, "QT": 2 * LR * TAU + 1e-6}

#         O  A   B   policy hidden critic hidden E  H  dropped G  Oc    lr_critic_delta
CASES = {
    "a_g1": (5, 2, 67, [64, 64], [64, 64], 3, 2, 2, 1, None, 0.0),
    "b_g3": (5, 2, 67, [64, 64], [64, 64], 3, 2, 2, 3, None, -2e-5),
    "c_one_value": (5, 2, 67, [64, 64], [64, 64], 1, 1, 0, 2, None, 0.0),
    "d_defaults": (5, 2, 64, [64, 64], [64, 64], 10, 2, 4, 2, None, 0.0),
    "e_critic_states": (12, 3, 70, [64, 64], [64, 64], 3, 2, 2, 2, 9, 0.0),
    "f_one_layer": (5, 2, 67, [64], [128], 3, 2, 2, 1, None, 0.0),
    "f_three_layers": (5, 2, 67, [64, 128, 64], [128, 64, 192], 3, 2, 2, 1, None, 0.0),
    "g_rows4096": (5, 2, 4096, [64, 64], [64, 64], 3, 2, 2, 2, None, 0.0),
    "h_rows4096_sixteen": (5, 2, 4096, [64, 64], [64, 64], 16, 2, 2, 2, None, 0.0),
}
# figures() of the twin in numpy float32 against the twin in float64, same inputs and noise (G > 1 and 4096 rows only).  Measured on
# a CPU; a figure missing here is below a tenth of its one-step bar: over the six cases metrics <= 8.3e-7, norms <= 4.4e-7, pm / qm
# <= 8.0e-7, la 9.8e-9, P99 / Q99 <= 3.0e-8, Pmax / Qmax <= 1.6e-6 (of 6.0e-4), QT below its relative part.  The second moments' 1.3e-5
# is float32's 1 - 0.999 (above), the same in every case.  Twice every gap is below its one-step bar: these cases meet the one-step bars.
F32_GAP = {
    "b_g3": {"pv": 1.30e-05, "qv": 1.28e-05},
    "c_one_value": {"pv": 1.29e-05, "qv": 1.26e-05},
    "d_defaults": {"pv": 1.30e-05, "qv": 1.29e-05},
    "e_critic_states": {"pv": 1.30e-05, "qv": 1.38e-05},
    "g_rows4096": {"pv": 1.32e-05, "qv": 1.33e-05},
    "h_rows4096_sixteen": {"pv": 1.26e-05, "qv": 1.30e-05},
}


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30))


def _hp(E, H, dropped, G, target_entropy=-1.0, delta=0.0):
    from rlx_amd.hip import AqeHparams
    return AqeHparams(GAMMA, TAU, target_entropy, -20.0, 2.0, LR, LR, delta, LR, 0.9, 0.999, 1e-8, E, H, dropped, G)


class Case:
    """name: a key of CASES -- or a row in CASES' form for a case of another table (tests/ens_cases.py), then called `label`, drawn from
    `seed` (the inputs) and seed + 1 (the noise), with no float32 gap until that table sets one (self.gap)"""

    def __init__(self, name, label=None, seed=None):
        O, A, B, ph, qh, E, H, dropped, G, Oc, delta = CASES[name] if isinstance(name, str) else name
        name = name if isinstance(name, str) else label
        self.name, self.O, self.A, self.B, self.E, self.H, self.dropped, self.G, self.delta = name, O, A, B, E, H, dropped, G, delta
        self.Oc = O if Oc is None else Oc
        self.gap = F32_GAP.get(name, {})
        p = tw.problem(O + B + G if seed is None else seed, O, A, B, ph, qh, E, H, dropped, G, Oc)
        self.ps, self.qs, self.state, self.batch, self.cbatch, self.h = p["ps"], p["qs"], p["state"], p["batch"], p["cbatch"], p["h"]
        rng = np.random.default_rng(7 + B if seed is None else seed + 1)
        self.eps = (rng.standard_normal((G, B, A)).astype(np.float32), rng.standard_normal((B, A)).astype(np.float32))
        self.pd = mlp_desc(O, ph, 2 * A, nets.ACT_RELU, False, False)
        self.qd = mlp_desc(self.Oc + A, qh, H, nets.ACT_RELU, False, False)

    def hp(self):
        return _hp(self.E, self.H, self.dropped, self.G, self.h["target_entropy"], self.delta)

    def chain(self, key, scheme):
        """the oracle's key chain (aqe.py:231-232, :245-246): G + 1 splits of count B + 1 -> (returned key, the key each step splits)"""
        part, step_keys = bool(scheme), []
        key = np.asarray(key, np.uint32)
        for _ in range(self.G + 1):
            step_keys.append(key)
            key = prng.split(key, self.B + 1, part)[0]
        return key, step_keys

    def twin(self, st, eps, dtype=np.float64):
        cb = self.cbatch or (None, None)
        st = {k: (np.asarray(v, np.float32).astype(dtype) if k in tw.STATE_KEYS else v) for k, v in st.items()}
        return tw.update(self.ps, self.qs, st, self.batch, eps[0], eps[1], self.h, LR, LR, self.delta, LR, TAU, cb[0], cb[1])


class Run:
    """one rlx_aqe_update_f32 call on device copies of a twin state"""

    def __init__(self, ctx, dev, c, st, key, scheme=1, inject=None, hp=None, prof=False):
        self.t = {k: _t(st[k], dev) for k in tw.STATE_KEYS}
        t = self.t
        met = torch.full((10,), 7.0, device=dev)
        hp = hp or c.hp()
        keep = [_t(x, dev) for x in c.cbatch] if c.cbatch else []
        if keep:
            hp.critic_states, hp.critic_next_states = keep[0].data_ptr(), keep[1].data_ptr()
        eps = None if inject is None else (_t(inject[0], dev), _t(inject[1], dev))     # kept alive: the library holds the pointers
        if eps is not None:
            ctx.dbg_set_sac_noise(*eps)
        if prof:
            ctx.prof_begin()
        try:
            self.key, self.q_count, self.pi_count = ctx.aqe_update(
                c.pd, t["P"], t["pm"], t["pv"], c.qd, t["Q"], t["qm"], t["qv"], t["QT"], t["la"], t["am"], t["av"],
                tuple(_t(x, dev) for x in c.batch), np.asarray(key, np.uint32), st["q_count"], st["pi_count"], hp, met, scheme)
        finally:
            ctx.dbg_set_sac_noise(None, None)
            if prof:
                ctx.prof_end()
        torch.cuda.synchronize()
        self.out = {k: v.cpu().numpy() for k, v in t.items()}
        self.metrics = met.cpu().numpy()

    def same_bits(self, other):
        return all(np.array_equal(self.out[k], other.out[k]) for k in tw.STATE_KEYS) and np.array_equal(self.metrics, other.metrics) \
            and np.array_equal(self.key, other.key)


def figures(out, metrics, new, met):
    """the one-step quantities as numbers: out / metrics of a run (or of the float32 twin) against the float64 twin"""
    exp = [float(met[n]) for n in NAMES] + [float(met["gradients/policy_grad_norm"]), float(met["gradients/critic_grad_norm"]),
                                            float(met["gradients/entropy_grad_norm"])]
    m = np.asarray(metrics, np.float64)
    f = {"metrics": max(abs(m[i] - exp[i]) / max(abs(exp[i]), 1.0) for i in (0, 1, 2, 3, 4, 5, 8)),
         "norms": max(abs(m[i] - exp[i]) / abs(exp[i]) for i in (6, 7))}
    for k in ("pm", "qm", "pv", "qv"):
        f[k] = _rel(out[k], new[k])
    f["la"] = abs(float(out["la"][0]) - float(new["la"][0]))
    for k in ("P", "Q"):
        d = np.abs(np.asarray(out[k], np.float64) - new[k])
        f[k + "99"], f[k + "max"] = float(np.quantile(d, 0.99)), float(d.max())
    f["QT"] = float((np.abs(np.asarray(out["QT"], np.float64) - new["QT"]) - 1e-4 * np.abs(new["QT"])).max())
    return f


def twin_metrics_vector(met):
    return [float(met[n]) for n in NAMES] + [float(met["gradients/policy_grad_norm"]), float(met["gradients/critic_grad_norm"]),
                                             float(met["gradients/entropy_grad_norm"]), 0.0]


def f32_gap(c):
    """the twin in numpy float32 against the twin in float64"""
    new, met, _, _ = c.twin(c.state, c.eps)
    new32, met32, _, _ = c.twin(c.state, c.eps, np.float32)
    return figures(new32, twin_metrics_vector(met32), new, met)


def check(c, r, new, met, label):
    f = figures(r.out, r.metrics, new, met)
    bars = {k: max(b, 2 * c.gap.get(k, 0.0)) for k, b in BARS.items()}
    print(f"aqe update {label}: " + " ".join(f"{k} {v:.2e}/{bars[k]:.1e}" for k, v in f.items()))
    assert r.metrics[9] == 0.0
    bad = {k: (v, bars[k]) for k, v in f.items() if not v <= bars[k]}
    assert not bad, bad


def _run_and_check(ctx, dev, name, scheme=1, prof=False):
    c = name if isinstance(name, Case) else Case(name)                             # (a Case of another table: tests/ens_cases.py)
    name = c.name
    r = Run(ctx, dev, c, c.state, KEY, scheme, inject=c.eps, prof=prof)
    key_e, _ = c.chain(KEY, scheme)
    assert np.array_equal(r.key, key_e)                                            # the oracle's chain: G + 1 splits of B + 1
    assert (r.q_count, r.pi_count) == (c.G, 1)
    new, met, g, ys = c.twin(c.state, c.eps)
    check(c, r, new, met, f"{name} scheme={scheme}")
    return c, r, new, met, g


@pytest.mark.parametrize("scheme", [1, 0])
def test_one_critic_step_matches_twin(ctx, dev, scheme):
    """case a -- O 5, A 2, B 67, hidden [64, 64], E 3, H 2, dropped 2, G 1: the one-step bars, under both threefry schemes"""
    assert "a_g1" not in F32_GAP
    _run_and_check(ctx, dev, "a_g1", scheme)


@pytest.mark.parametrize("name", ["f_one_layer", "f_three_layers"])
def test_other_depths_match_twin(ctx, dev, name):
    """case f -- one hidden layer; three unequal ones: G 1, the one-step bars"""
    assert name not in F32_GAP
    _run_and_check(ctx, dev, name)


@pytest.mark.parametrize("name", ["b_g3", "c_one_value", "d_defaults", "e_critic_states"])
def test_several_critic_steps_match_twin(ctx, dev, name):
    c, r, new, met, g = _run_and_check(ctx, dev, name)
    # metrics [0] and [7] are the means over the steps (aqe.py:242): the last step alone would read differently
    norms = [np.linalg.norm(x) for x in g["gq"]]
    assert r.metrics[7] == pytest.approx(np.mean(norms), rel=1e-5)
    assert abs(norms[-1] - np.mean(norms)) > 1e-3 * np.mean(norms)
    assert r.metrics[0] == pytest.approx(float(met["loss/q_loss"]), rel=1e-5, abs=1e-5)


def test_second_call_from_nonzero_moments_and_counts(ctx, dev):
    """a second call from the twin's state after the first: non-zero moments in all three optimisers, counters (3, 1) -> (6, 2)"""
    c = Case("b_g3")
    new, _, _, _ = c.twin(c.state, c.eps)
    st1 = {k: (np.asarray(v, np.float32).astype(np.float64) if k in tw.STATE_KEYS else v) for k, v in new.items()}
    assert (st1["q_count"], st1["pi_count"]) == (3, 1) and all(np.any(st1[k] != 0) for k in ("pm", "pv", "qm", "qv", "am", "av"))
    r2 = Run(ctx, dev, c, st1, prng.prng_key(12), 1, inject=c.eps)
    assert (r2.q_count, r2.pi_count) == (6, 2)
    new2, met2, _, _ = c.twin(st1, c.eps)
    check(c, r2, new2, met2, "b_g3, second call")


def _hidden_launches(c):
    # per critic step: policy 1, targets E, online E; policy step: policy 1, online E
    return c.G * (1 + 2 * c.E) + 1 + c.E


def test_rows_4096_split_operand_engine_and_image_rebuild(ctx, dev):
    """case g -- 4096 rows: the hidden layers take the split-operand images, rebuilt in front of every critic step from the
    parameters the previous step left (stale images would evaluate step 2 with step 1's critics: lr per weight, far outside the
    bars).  Every 64 x 64 forward launch ran on engine 1; the first layers, whose 5 and 7 input columns are no multiple of four, have
    no image and stay on the exact engine (trunk_images)"""
    c, r, _, _, _ = _run_and_check(ctx, dev, "g_rows4096", prof=True)
    rows = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    print("aqe 4096 gemm rows:", [(q["kernel"], q["engine"], q["M"], q["N"], q["K"], q["launches"]) for q in rows])
    if ctx.get_counter("gemm_bx") != 1:
        assert all(q["engine"] == 0 for q in rows), rows
        return
    hidden = [q for q in rows if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (4096, 64, 64)]
    assert hidden and {q["engine"] for q in hidden} == {1} and sum(q["launches"] for q in hidden) == _hidden_launches(c), hidden
    first = [q for q in rows if q["kernel"] == "k_gemm_fwd" and q["K"] in (5, 7)]
    assert first and {q["engine"] for q in first} == {0}, first


def test_rows_4096_sixteen_critics_overflow_the_image_job_table(ctx, dev):
    """case h -- 4096 rows, 16 critics: a critic step lists 1 + 3 E = 49 images for the builder's job table; the list ends inside
    the critics and the rest run their hidden layers on the exact engine (net_pass.h: trunk_images) -- same results, same bars"""
    c, r, _, _, _ = _run_and_check(ctx, dev, "h_rows4096_sixteen", prof=True)
    if ctx.get_counter("gemm_bx") != 1:
        return
    hidden = [q for q in ctx.prof_rows() if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (4096, 64, 64)]
    print("aqe 4096 x 16 hidden forward rows:", [(q["engine"], q["launches"]) for q in hidden])
    assert {q["engine"] for q in hidden} == {0, 1}, hidden
    assert sum(q["launches"] for q in hidden) == _hidden_launches(c)


def test_two_identical_calls_give_identical_bits(ctx, dev):
    for name in ("b_g3", "g_rows4096"):
        c = Case(name)
        assert Run(ctx, dev, c, c.state, KEY).same_bits(Run(ctx, dev, c, c.state, KEY)), name
        assert Run(ctx, dev, c, c.state, KEY, inject=c.eps).same_bits(Run(ctx, dev, c, c.state, KEY, inject=c.eps)), name


@pytest.mark.parametrize("scheme", [1, 0])
def test_keyed_noise_equals_the_oracle_draw(ctx, dev, scheme):
    """without the hook the noise comes from the keys: row b of every step, critic or policy, draws normal(split(key_i, B + 1)[1 + b],
    (A,)).  The device's normal() and the oracle's agree to a few float32 ulps, not bit for bit: the keyed run meets the bars against
    the twin on the oracle's draws, and equals the run they are injected into"""
    c = Case("b_g3")
    part = bool(scheme)
    key_e, step_keys = c.chain(KEY, scheme)
    draw = lambda k: np.stack([prng.normal(kk, (c.A,), part) for kk in prng.split(k, c.B + 1, part)[1:]])
    e1, e2 = np.stack([draw(step_keys[i]) for i in range(c.G)]), draw(step_keys[c.G])
    keyed = Run(ctx, dev, c, c.state, KEY, scheme)
    assert np.array_equal(keyed.key, key_e)
    new, met, _, _ = c.twin(c.state, (e1, e2))
    check(c, keyed, new, met, f"keyed scheme={scheme}")
    inj = Run(ctx, dev, c, c.state, KEY, scheme, inject=(e1, e2))
    assert np.array_equal(inj.key, keyed.key)
    assert _rel(inj.out["pm"], keyed.out["pm"].astype(np.float64)) < 1e-5 and _rel(inj.out["qm"], keyed.out["qm"].astype(np.float64)) < 1e-5
    # other noise gives another update: the hook is read, and step i reads rows [i B, (i + 1) B) of it
    other = Run(ctx, dev, c, c.state, KEY, scheme, inject=(e1[::-1].copy(), e2))
    assert _rel(other.out["qm"], keyed.out["qm"].astype(np.float64)) > 1e-3


@pytest.mark.parametrize("what,code,word", [
    ("hidden96", -4, "hidden widths"), ("tanh", -1, "RLX_ACT_RELU"), ("ln_first", -1, "ln_first"), ("out_dim", -1, "qdesc->out_dim"),
    ("a65", -4, "act_dim"), ("t129", -4, "at most 128"), ("dropped_t", -1, "nr_dropped_q_values"), ("g65", -4, "q_update_steps"),
    ("g0", -1, "q_update_steps"), ("e17", -4, "ensemble_size"), ("one_critic_pointer", -1, "critic_states")])
def test_refusals_leave_the_outputs_alone(ctx, dev, what, code, word):
    O, A, E, H, dropped, G, qout, hidden, act, ln = 8, 2, 3, 2, 2, 2, 2, [64, 64], nets.ACT_RELU, False
    if what == "hidden96":
        hidden = [64, 96]
    elif what == "tanh":
        act = nets.ACT_TANH
    elif what == "ln_first":
        ln = True
    elif what == "out_dim":
        qout = 3
    elif what == "a65":
        A = 65
    elif what == "t129":
        E, H, qout = 3, 43, 43
    elif what == "dropped_t":
        dropped = 6
    elif what == "g65":
        G = 65
    elif what == "g0":
        G = 0
    elif what == "e17":
        E = 17
    pd = mlp_desc(O, [64, 64], 2 * A, nets.ACT_RELU, False, False)
    qd = mlp_desc(O + A, hidden, qout, act, ln, False)
    hp = _hp(E, H, dropped, G)
    x = torch.zeros(256, device=dev)                                  # B = 256 / G rows: positive at G = 65 too
    if what == "one_critic_pointer":
        hp.critic_states = x.data_ptr()
    key = np.array(KEY, np.uint32)
    with pytest.raises(RlxError) as e:
        ctx.aqe_update(pd, x, x, x, qd, x, x, x, x, x, x, x, (x, x, x, x, x), key, 0, 0, hp, x)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(x).item() == 0


if __name__ == "__main__":      # the float32 gaps behind F32_GAP (CPU only)
    for name in F32_GAP:
        gap = f32_gap(Case(name))
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in gap.items() if v > 0.1 * BARS[k]) + "},")
        print("      # all:", " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
