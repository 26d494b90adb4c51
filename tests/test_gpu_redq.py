"""GPU: rlx_redq_update_f32 -- the whole REDQ update, G critic steps and one policy step -- against the float64 twin
(tests/redq_twin.py) on the same float32 inputs, with the noise injected through rlx_dbg_set_sac_noise and the library's target
subsets (subsets_out, themselves checked against oracle/prng.py) fed to the twin.

Inputs: tests/test_gpu_tqc.py's recipe (tw.problem).  Figures (figures()) and their bars for ONE critic step (BARS) are
tests/test_gpu_tqc.py::check_first_step's, restated: metrics 1e-5 relative and absolute, the two norms 1e-5 relative; first moments
(a first step's are gradients / 10) 1e-5 relative L2; parameter steps within 2e-5 on 99 % of the entries and within 2 lr + 1e-6
everywhere; log_alpha 1e-6; targets rtol 1e-4, atol 2 lr tau + 1e-6.  check_first_step has no bar for the second moments; theirs is
check_second_step's of the same file, 5e-5 relative L2 (float32's 1 - 0.999 is 1.29e-5 off 0.001, in every float32 Adam).

Several critic steps, and 4096 rows, compound float32 rounding: the twin evaluated in numpy float32 on the same inputs is itself off
the float64 twin by F32_GAP below (measured once on a CPU: this file run as a script, repository root and rl-x_amd on PYTHONPATH).
Those cases are held to twice that gap or to the one-step bar, whichever is larger."""
import numpy as np
import pytest
import torch

import redq_twin as tw
from oracle import nets, prng
from rlx_amd.hip import RedqHparams, RlxError, mlp_desc, redq_subset

pytestmark = pytest.mark.gpu

GAMMA, TAU, LR = 0.99, 0.005, 3e-4
NAMES = tw.METRICS
KEY = prng.prng_key(11)

BARS = {"metrics": 1e-5, "norms": 1e-5, "pm": 1e-5, "qm": 1e-5, "pv": 5e-5, "qv": 5e-5, "la": 1e-6, "P99": 2e-5, "Q99": 2e-5,
        "Pmax": 2 * LR + 1e-6, "Qmax": 2 * LR + 1e-6, "QT": 2 * LR * TAU + 1e-6}

#         O  A   B   policy hidden critic hidden E  M  G  Oc    lr_critic_delta
CASES = {
    "g1": (5, 2, 67, [64, 64], [64, 64], 3, 2, 1, None, 0.0),
    "g3": (5, 2, 67, [64, 64], [64, 64], 3, 2, 3, None, -2e-5),
    "one_net": (5, 2, 67, [64, 64], [64, 64], 1, 1, 2, None, 0.0),
    "ten_nets": (5, 2, 64, [64, 64], [64, 64], 10, 2, 2, None, 0.0),
    "critic_states": (12, 3, 70, [64, 64], [64, 64], 3, 2, 2, 9, 0.0),
    "rows4096": (5, 2, 4096, [64, 64], [64, 64], 3, 2, 2, None, 0.0),
    "rows4096_sixteen": (5, 2, 4096, [64, 64], [64, 64], 16, 2, 2, None, 0.0),
}
# figures() of the twin in numpy float32 against the twin in float64, same inputs, noise and subsets (G > 1 and 4096 rows only).
# Measured on a CPU; a figure missing here is below a tenth of its one-step bar: over the six cases metrics <= 2.2e-7, norms <= 1.3e-7,
# pm / qm <= 4.0e-7, la 9.8e-9, P99 / Q99 <= 3.0e-8, Pmax / Qmax <= 4.3e-7, QT below its relative part.  The second moments' 1.3e-5 is
# float32's 1 - 0.999 (above), the same in every case.  Twice every gap is below its one-step bar: these cases meet the one-step bars.
F32_GAP = {
    "g3": {"pv": 1.29e-05, "qv": 1.26e-05},
    "one_net": {"pv": 1.29e-05, "qv": 1.26e-05},
    "ten_nets": {"pv": 1.27e-05, "qv": 1.28e-05},
    "critic_states": {"pv": 1.31e-05, "qv": 1.30e-05},
    "rows4096": {"pv": 1.28e-05, "qv": 1.30e-05},
    "rows4096_sixteen": {"pv": 1.27e-05, "qv": 1.30e-05},
}


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30))


class Case:
    """name: a key of CASES -- or a row in CASES' form for a case of another table (tests/ens_cases.py), then called `label`, drawn from
    `seed` (the inputs) and seed + 1 (the noise), with no float32 gap until that table sets one (self.gap)"""

    def __init__(self, name, label=None, seed=None):
        O, A, B, ph, qh, E, M, G, Oc, delta = CASES[name] if isinstance(name, str) else name
        name = name if isinstance(name, str) else label
        self.name, self.O, self.A, self.B, self.E, self.M, self.G, self.Oc, self.delta = name, O, A, B, E, M, G, O if Oc is None else Oc, delta
        self.gap = F32_GAP.get(name, {})
        p = tw.problem(O + B + G if seed is None else seed, O, A, B, ph, qh, E, M, G, Oc)
        self.ps, self.qs, self.state, self.batch, self.cbatch, self.h = p["ps"], p["qs"], p["state"], p["batch"], p["cbatch"], p["h"]
        rng = np.random.default_rng(7 + B if seed is None else seed + 1)
        self.eps = (rng.standard_normal((G, B, A)).astype(np.float32), rng.standard_normal((B, A)).astype(np.float32))
        self.pd = mlp_desc(O, ph, 2 * A, nets.ACT_RELU, False, False)
        self.qd = mlp_desc(self.Oc + A, qh, 1, nets.ACT_RELU, False, False)

    def hp(self):
        return RedqHparams(GAMMA, TAU, self.h["target_entropy"], -20.0, 2.0, LR, LR, self.delta, LR, 0.9, 0.999, 1e-8, self.E, self.M, self.G)

    def chain(self, key, scheme):
        """the oracle's key chain (redq.py:229-230, :247-248) -> (returned key, the G sample keys, the key each step splits)"""
        part, sks, step_keys = bool(scheme), [], []
        key = np.asarray(key, np.uint32)
        for _ in range(self.G):
            step_keys.append(key)
            ks = prng.split(key, self.B + 2, part)
            key, sk = ks[0], ks[1]
            sks.append(sk)
        step_keys.append(key)
        return prng.split(key, self.B + 1, part)[0], sks, step_keys

    def subsets(self, key, scheme):
        return np.array([prng.permutation_rows(sk, np.arange(self.E)[None], bool(scheme))[0, :self.M] for sk in self.chain(key, scheme)[1]])

    def twin(self, st, eps, subsets, dtype=np.float64):
        cb = self.cbatch or (None, None)
        st = {k: (np.asarray(v, np.float32).astype(dtype) if k in tw.STATE_KEYS else v) for k, v in st.items()}
        return tw.update(self.ps, self.qs, st, self.batch, eps[0], eps[1], subsets, self.h, LR, LR, self.delta, LR, TAU, cb[0], cb[1])


class Run:
    """one rlx_redq_update_f32 call on device copies of a twin state"""

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
            self.key, self.q_count, self.pi_count, self.subsets = ctx.redq_update(
                c.pd, t["P"], t["pm"], t["pv"], c.qd, t["Q"], t["qm"], t["qv"], t["QT"], t["la"], t["am"], t["av"],
                tuple(_t(x, dev) for x in c.batch), np.asarray(key, np.uint32), st["q_count"], st["pi_count"], hp, met, scheme, subsets=True)
        finally:
            ctx.dbg_set_sac_noise(None, None)
            if prof:
                ctx.prof_end()
        torch.cuda.synchronize()
        self.out = {k: v.cpu().numpy() for k, v in t.items()}
        self.metrics = met.cpu().numpy()

    def same_bits(self, other):
        return all(np.array_equal(self.out[k], other.out[k]) for k in tw.STATE_KEYS) and np.array_equal(self.metrics, other.metrics) \
            and np.array_equal(self.key, other.key) and np.array_equal(self.subsets, other.subsets)


def figures(out, metrics, new, met):
    """check_first_step's quantities as numbers: out / metrics of a run (or of the float32 twin) against the float64 twin"""
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
    """the twin in numpy float32 against the twin in float64 (the subsets are the oracle's for KEY)"""
    sub = c.subsets(KEY, 1)
    new, met, _, _ = c.twin(c.state, c.eps, sub)
    new32, met32, _, _ = c.twin(c.state, c.eps, sub, np.float32)
    return figures(new32, twin_metrics_vector(met32), new, met)


def check(c, r, new, met, label):
    f = figures(r.out, r.metrics, new, met)
    bars = {k: max(b, 2 * c.gap.get(k, 0.0)) for k, b in BARS.items()}
    print(f"redq update {label}: " + " ".join(f"{k} {v:.2e}/{bars[k]:.1e}" for k, v in f.items()))
    assert r.metrics[9] == 0.0
    bad = {k: (v, bars[k]) for k, v in f.items() if not v <= bars[k]}
    assert not bad, bad


def _run_and_check(ctx, dev, name, scheme=1, prof=False):
    c = name if isinstance(name, Case) else Case(name)                             # (a Case of another table: tests/ens_cases.py)
    name = c.name
    r = Run(ctx, dev, c, c.state, KEY, scheme, inject=c.eps, prof=prof)
    key_e, sks, _ = c.chain(KEY, scheme)
    assert np.array_equal(r.key, key_e)                                            # the oracle's chain: G splits of B + 2, one of B + 1
    assert (r.q_count, r.pi_count) == (c.G, 1)
    assert r.subsets.shape == (c.G, c.M)
    for i, sk in enumerate(sks):
        assert np.array_equal(r.subsets[i], redq_subset(sk, c.E, c.M, scheme)), i
    assert np.array_equal(r.subsets, c.subsets(KEY, scheme))
    new, met, g, ys = c.twin(c.state, c.eps, r.subsets)
    check(c, r, new, met, f"{name} scheme={scheme}")
    return c, r, new, met, g


@pytest.mark.parametrize("scheme", [1, 0])
def test_one_critic_step_matches_twin(ctx, dev, scheme):
    """O 5, A 2, B 67, hidden [64, 64], E 3, M 2, G 1: check_first_step's bars"""
    assert "g1" not in F32_GAP
    _run_and_check(ctx, dev, "g1", scheme)


@pytest.mark.parametrize("name", ["g3", "one_net", "ten_nets", "critic_states"])
def test_several_critic_steps_match_twin(ctx, dev, name):
    c, r, new, met, g = _run_and_check(ctx, dev, name)
    # metrics [0] and [7] are the means over the steps (redq.py:244): the last step alone would read differently
    norms = [np.linalg.norm(x) for x in g["gq"]]
    assert r.metrics[7] == pytest.approx(np.mean(norms), rel=1e-5)
    assert abs(norms[-1] - np.mean(norms)) > 1e-3 * np.mean(norms)
    assert r.metrics[0] == pytest.approx(float(met["loss/q_loss"]), rel=1e-5, abs=1e-5)


def test_second_call_from_nonzero_moments_and_counts(ctx, dev):
    """a second call from the twin's state after the first: non-zero moments in all three optimisers, counters (3, 1) -> (6, 2)"""
    c = Case("g3")
    sub = c.subsets(KEY, 1)
    new, _, _, _ = c.twin(c.state, c.eps, sub)
    st1 = {k: (np.asarray(v, np.float32).astype(np.float64) if k in tw.STATE_KEYS else v) for k, v in new.items()}
    assert (st1["q_count"], st1["pi_count"]) == (3, 1) and all(np.any(st1[k] != 0) for k in ("pm", "pv", "qm", "qv", "am", "av"))
    key2 = prng.prng_key(12)
    r2 = Run(ctx, dev, c, st1, key2, 1, inject=c.eps)
    assert (r2.q_count, r2.pi_count) == (6, 2)
    new2, met2, _, _ = c.twin(st1, c.eps, r2.subsets)
    check(c, r2, new2, met2, "g3, second call")


def test_rows_4096_split_operand_engine_and_image_rebuild(ctx, dev):
    """4096 rows: the hidden layers take the split-operand images, rebuilt in front of every critic step from the parameters the
    previous step left (stale images would evaluate step 2 with step 1's critics: lr per weight, far outside the bars).  The first
    layers, whose 5 and 7 input columns are no multiple of four, have no image and stay on the exact engine (trunk_images)"""
    c, r, _, _, _ = _run_and_check(ctx, dev, "rows4096", prof=True)
    rows = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    print("redq 4096 gemm rows:", [(q["kernel"], q["engine"], q["M"], q["N"], q["K"], q["launches"]) for q in rows])
    if ctx.get_counter("gemm_bx") != 1:
        assert all(q["engine"] == 0 for q in rows), rows
        return
    hidden = [q for q in rows if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (4096, 64, 64)]
    # per critic step: policy 1, targets M, online E; policy step: policy 1, online E
    assert hidden and {q["engine"] for q in hidden} == {1} and sum(q["launches"] for q in hidden) == c.G * (1 + c.M + c.E) + 1 + c.E, hidden
    first = [q for q in rows if q["kernel"] == "k_gemm_fwd" and q["K"] in (5, 7)]
    assert first and {q["engine"] for q in first} == {0}, first


def test_rows_4096_sixteen_critics_overflow_the_image_job_table(ctx, dev):
    """4096 rows, 16 critics: a critic step lists 1 + M + 2 E = 35 images for the builder's 32 jobs; the list ends inside the online
    critics and the last ones run their hidden layers on the exact engine (net_pass.h: trunk_images) -- same results, same bars"""
    c, r, _, _, _ = _run_and_check(ctx, dev, "rows4096_sixteen", prof=True)
    if ctx.get_counter("gemm_bx") != 1:
        return
    hidden = [q for q in ctx.prof_rows() if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (4096, 64, 64)]
    print("redq 4096 x 16 hidden forward rows:", [(q["engine"], q["launches"]) for q in hidden])
    assert {q["engine"] for q in hidden} == {0, 1}, hidden
    assert sum(q["launches"] for q in hidden) == c.G * (1 + c.M + c.E) + 1 + c.E


def test_two_identical_calls_give_identical_bits(ctx, dev):
    for name in ("g3", "rows4096"):
        c = Case(name)
        assert Run(ctx, dev, c, c.state, KEY).same_bits(Run(ctx, dev, c, c.state, KEY)), name
        assert Run(ctx, dev, c, c.state, KEY, inject=c.eps).same_bits(Run(ctx, dev, c, c.state, KEY, inject=c.eps)), name


@pytest.mark.parametrize("scheme", [1, 0])
def test_keyed_noise_equals_the_oracle_draw(ctx, dev, scheme):
    """without the hook the noise comes from the keys: row b of critic step i draws normal(split(key_i, B + 2)[2 + b], (A,)), row b
    of the policy step normal(split(key_G, B + 1)[1 + b], (A,)).  The device's normal() and the oracle's agree to a few float32 ulps,
    not bit for bit: the keyed run meets the bars against the twin on the oracle's draws, and equals the run they are injected into"""
    c = Case("g3")
    part = bool(scheme)
    _, _, step_keys = c.chain(KEY, scheme)
    e1 = np.stack([np.stack([prng.normal(k, (c.A,), part) for k in prng.split(step_keys[i], c.B + 2, part)[2:]]) for i in range(c.G)])
    e2 = np.stack([prng.normal(k, (c.A,), part) for k in prng.split(step_keys[c.G], c.B + 1, part)[1:]])
    keyed = Run(ctx, dev, c, c.state, KEY, scheme)
    new, met, _, _ = c.twin(c.state, (e1, e2), keyed.subsets)
    check(c, keyed, new, met, f"keyed scheme={scheme}")
    inj = Run(ctx, dev, c, c.state, KEY, scheme, inject=(e1, e2))
    assert np.array_equal(inj.key, keyed.key) and np.array_equal(inj.subsets, keyed.subsets)
    assert _rel(inj.out["pm"], keyed.out["pm"].astype(np.float64)) < 1e-5 and _rel(inj.out["qm"], keyed.out["qm"].astype(np.float64)) < 1e-5
    # other noise gives another update: the hook is read, and step i reads rows [i B, (i + 1) B) of it
    other = Run(ctx, dev, c, c.state, KEY, scheme, inject=(e1[::-1].copy(), e2))
    assert _rel(other.out["qm"], keyed.out["qm"].astype(np.float64)) > 1e-3


@pytest.mark.parametrize("what,code,word", [
    ("m_above_e", -1, "in_target_minimization_size"), ("e17", -4, "ensemble_size"), ("g0", -1, "q_update_steps"),
    ("out_dim", -1, "qdesc->out_dim"), ("one_critic_pointer", -1, "critic_states")])
def test_refusals_leave_the_outputs_alone(ctx, dev, what, code, word):
    O, A, E, M, G, qout = 8, 2, 3, 2, 2, 1
    if what == "m_above_e":
        M = 4
    elif what == "e17":
        E, M = 17, 2
    elif what == "g0":
        G = 0
    elif what == "out_dim":
        qout = 2
    pd = mlp_desc(O, [64, 64], 2 * A, nets.ACT_RELU, False, False)
    qd = mlp_desc(O + A, [64, 64], qout, nets.ACT_RELU, False, False)
    hp = RedqHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, 0.0, LR, 0.9, 0.999, 1e-8, E, M, G)
    x = torch.zeros(64, device=dev)
    if what == "one_critic_pointer":
        hp.critic_states = x.data_ptr()
    with pytest.raises(RlxError) as e:
        ctx.redq_update(pd, x, x, x, qd, x, x, x, x, x, x, x, (x, x, x, x, x), KEY, 0, 0, hp, x)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(x).item() == 0


if __name__ == "__main__":      # the float32 gaps behind F32_GAP (CPU only)
    for name in F32_GAP:
        gap = f32_gap(Case(name))
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in gap.items() if v > 0.1 * BARS[k]) + "},")
        print("      # all:", " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
