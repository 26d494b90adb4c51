"""GPU: rlx_tqc_update_f32 -- the whole TQC update -- against the float64 twin (tests/tqc_twin.py) on the same float32 inputs.

The input recipe and the bars are tests/test_gpu_sac.py::test_sac_update_matches_oracle's at head_scale 0.1: metrics 1e-5 relative
and absolute; gradient vectors (first-step first moments x 10) 1e-5 relative L2; parameter steps within 2e-5 on >= 99 % of the
entries and within 2 lr + 1e-6 everywhere; log_alpha 1e-6; targets rtol 1e-4, atol 2 lr tau + 1e-6.  The second step's bars are
tests/test_gpu_mpo_shapes.py's (mpo_cases.UPDATED): parameters and first moments 1e-5 relative L2, second moments 5e-5."""
import numpy as np
import pytest
import torch

import tqc_twin as tw
from oracle import nets, prng, sac
from rlx_amd.hip import RlxError, TqcHparams, mlp_desc

pytestmark = pytest.mark.gpu

GAMMA, TAU, LR = 0.99, 0.005, 3e-4
NAMES = tw.METRICS


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30))


class Case:
    """test_sac_update_matches_oracle's inputs (head_scale 0.1) for E critics of N atoms; Oc: the critics' own observation width"""

    def __init__(self, O, A, B, ph, qh, E, N, dropped, Oc=None, kappa=1.0, seed=None):
        self.O, self.A, self.B, self.E, self.N, self.dropped, self.ph, self.qh = O, A, B, E, N, dropped, list(ph), list(qh)
        self.Oc = O if Oc is None else Oc
        rng = np.random.default_rng(O + B if seed is None else seed)
        self.ps, self.qs = ps, qs = tw.make_specs(O, self.Oc, A, self.ph, self.qh, N)
        pp = (sac.lecun_normal_init(ps, rng) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
        pp[ps.head["W"]:ps.head["W"] + ps.head["in"] * ps.head["out"]] *= 0.1
        qp = (np.concatenate([sac.lecun_normal_init(qs, rng) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params)).astype(np.float32)
        qtp = (qp + 0.01 * rng.standard_normal(qp.shape)).astype(np.float32)
        f = lambda x: x.astype(np.float32)
        self.batch = (f(rng.standard_normal((B, O))), f(rng.standard_normal((B, O))), f(np.tanh(rng.standard_normal((B, A)))),
                      f(rng.standard_normal(B)), f(rng.random(B) < 0.2))
        self.cbatch = None if Oc is None else (f(rng.standard_normal((B, Oc))), f(rng.standard_normal((B, Oc))))
        self.state = tw.zero_state(pp, qp, qtp, np.float32(-0.3))
        self.h = dict(gamma=GAMMA, target_entropy=-float(A), ensemble_size=E, nr_atoms_per_net=N, nr_dropped_atoms_per_net=dropped,
                      huber_kappa=kappa, log_std_min=-20.0, log_std_max=2.0)
        self.pd = mlp_desc(O, self.ph, 2 * A, nets.ACT_RELU, False, False)
        self.qd = mlp_desc(self.Oc + A, self.qh, N, nets.ACT_RELU, False, False)

    def hp(self):
        h = self.h
        return TqcHparams(GAMMA, TAU, h["target_entropy"], -20.0, 2.0, LR, LR, LR, 0.9, 0.999, 1e-8, h["huber_kappa"], self.E, self.N, self.dropped)

    def twin(self, st, eps, dtype=np.float64):
        """-> tw.update's (new state, metrics, gradients, aux); dtype: the arithmetic of the whole evaluation (the state's float32
        values in it)"""
        cb = self.cbatch or (None, None)
        f = lambda x: None if x is None else x.astype(dtype)
        if dtype != np.float64:
            st = {k: (np.asarray(v, np.float32).astype(dtype) if k in tw.STATE_KEYS else v) for k, v in st.items()}
        return tw.update(self.ps, self.qs, st, tuple(f(x) for x in self.batch), f(eps[0]), f(eps[1]), self.h, LR, TAU, f(cb[0]), f(cb[1]))


class Run:
    """one rlx_tqc_update_f32 call on device copies of a twin state"""

    def __init__(self, ctx, dev, c, st, key, scheme=1, inject=None, prof=False):
        self.t = {k: _t(st[k], dev) for k in tw.STATE_KEYS}
        t = self.t
        met = torch.full((10,), 7.0, device=dev)
        hp = c.hp()
        keep = [_t(x, dev) for x in c.cbatch] if c.cbatch else []
        if keep:
            hp.critic_states, hp.critic_next_states = keep[0].data_ptr(), keep[1].data_ptr()
        eps = None if inject is None else (_t(inject[0], dev), _t(inject[1], dev))     # kept alive: the library holds the pointers
        if eps is not None:
            ctx.dbg_set_sac_noise(*eps)
        if prof:
            ctx.prof_begin()
        try:
            self.key, self.count = ctx.tqc_update(c.pd, t["P"], t["pm"], t["pv"], c.qd, t["Q"], t["qm"], t["qv"], t["QT"], t["la"], t["am"], t["av"],
                                                  tuple(_t(x, dev) for x in c.batch), np.asarray(key, np.uint32), st["count"], hp, met, scheme)
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


def check_first_step(r, new, met, grads, label):
    """the bars of test_sac_update_matches_oracle at head_scale 0.1, for a step from zero moments"""
    gp, gq, ga = grads
    m = r.metrics
    figures = {n.split("/")[1]: abs(m[i] - float(met[n])) / max(abs(float(met[n])), 1e-30) for i, n in enumerate(NAMES)}
    rp, rq = _rel(r.out["pm"] * 10, gp), _rel(r.out["qm"] * 10, gq)
    print(f"tqc update {label}: ||dg||/||g|| policy {rp:.2e} critic {rq:.2e}; " + " ".join(f"{k} {v:.1e}" for k, v in figures.items()))
    for i, n in enumerate(NAMES):
        assert m[i] == pytest.approx(float(met[n]), rel=1e-5, abs=1e-5), n
    assert m[6] == pytest.approx(np.linalg.norm(gp), rel=1e-5)
    assert m[7] == pytest.approx(np.linalg.norm(gq), rel=1e-5)
    assert m[8] == pytest.approx(abs(float(ga)), rel=1e-5, abs=1e-5)
    assert m[9] == 0.0
    assert rp < 1e-5 and rq < 1e-5
    assert float(r.out["la"][0]) == pytest.approx(new["la"][0], abs=1e-6)
    for k in ("P", "Q"):
        d = np.abs(r.out[k] - new[k])
        assert (d <= 2e-5).mean() > 0.99 and d.max() <= 2 * LR + 1e-6, k
    np.testing.assert_allclose(r.out["QT"], new["QT"], rtol=1e-4, atol=2 * LR * TAU + 1e-6)


KINK, MAX_FLIPS = 8e-6, 3
# The 4096-row case against the PLAIN float64 twin: the twin itself evaluated in numpy float32 on the same inputs is 1.73e-5 off in
# the critic gradient (8.6e-4 / 6.3e-5 in W1 / W2 of critic 0, 2e-7 .. 3e-7 in every other block; policy 2.0e-7): unit 35 of
# critic 0's second layer sits at |z| / rms = 1.2e-7 for row 3954 and float32 puts it on the other side of its kink.  float32
# cannot meet 1e-5 there; the bar derived from that gap is twice it.
F32_GAP_4096 = 1.73e-5


def admissible_critic_gradient(c, r, gq, aux, label):
    """tests/test_gpu_bench_shapes.py's rule for a batch of millions of unit-samples: a ReLU unit whose float64 pre-activation
    sits within float32 rounding of zero for some sample (|z| < KINK of the row's RMS: a 256-term float32 dot product) may be on in
    one float32 evaluation and off in another, and that sample's contribution through the unit flips with it.  Such units of the
    online critics on (s, a) are found from the float64 pre-activations alone, closest first; the device's gradient has to agree
    with the twin's for SOME on / off assignment of at most MAX_FLIPS of them (samples contribute independently: the deltas add)
    -> that assignment's gradient, which then meets the same bars.  Against the plain twin the gradient is held to twice the
    float32-vs-float64 gap of the twin itself (F32_GAP_4096)."""
    got = r.out["qm"].astype(np.float64) * 10
    assert _rel(got, gq) < 2 * F32_GAP_4096, _rel(got, gq)
    if _rel(got, gq) < 1e-6:
        return gq
    n, N = c.qs.n_params, c.N
    cs = c.batch[0] if c.cbatch is None else c.cbatch[0]
    x = np.concatenate([cs, c.batch[2]], axis=1).astype(np.float64)
    cand = [(e,) + k for e in range(c.E) for k in tw.kink_entries(c.qs, c.state["Q"][e * n:(e + 1) * n], x, KINK)]
    cand.sort(key=lambda k: k[4])
    adm, taken = gq.copy(), []
    for e, layer, row, unit, dist in cand:
        if _rel(got, adm) < 1e-6:
            break
        trial = adm.copy()
        trial[e * n:(e + 1) * n] += tw.critic_kink_delta(c.qs, c.state["Q"][e * n:(e + 1) * n], x[row:row + 1],
                                                         aux["dq"][row:row + 1, e * N:(e + 1) * N], layer, unit)
        if _rel(got, trial) < 0.9 * _rel(got, adm):
            adm, taken = trial, taken + [(e, layer, row, unit, float(f"{dist:.1e}"))]
    print(f"tqc update {label}: critic gradient vs the plain twin {_rel(got, gq):.2e}; {len(cand)} unit-samples within {KINK:.0e} of the ReLU "
          f"kink; on the other side on the device (critic, layer, row, unit, |z|/rms): {taken} -> {_rel(got, adm):.2e}")
    assert len(taken) <= MAX_FLIPS, taken
    return adm


def check_second_step(r, new):
    """tests/test_gpu_mpo_shapes.py's second step (mpo_cases.UPDATED): parameters and first moments 1e-5, second moments 5e-5"""
    bars = (("P", 1e-5), ("pm", 1e-5), ("pv", 5e-5), ("Q", 1e-5), ("qm", 1e-5), ("qv", 5e-5), ("la", 1e-5), ("am", 1e-5), ("av", 5e-5),
            ("QT", 1e-5))
    bad = [(k, _rel(r.out[k], new[k])) for k, tol in bars if not _rel(r.out[k], new[k]) < tol]
    assert not bad, bad


#           O   A    B   policy hidden  critic hidden   E   N  dropped
CASES = {
    "tiny": (3, 1, 64, [64, 64], [64, 64], 2, 25, 2),
    "five_nets": (11, 3, 200, [64, 64], [64, 64], 5, 25, 2),
    "no_drop": (45, 5, 130, [128, 128], [128, 128], 3, 7, 0),
    "one_net_128": (40, 6, 100, [64, 64], [64, 64], 1, 128, 5),
    "defaults": (376, 17, 256, [256, 256], [256, 256], 2, 25, 2),
    "one_hidden": (20, 4, 96, [64], [128], 2, 25, 2),
    "three_hidden": (20, 4, 96, [128, 64, 64], [64, 128, 64], 2, 25, 2),
}
SMALL = ["tiny", "five_nets", "no_drop", "one_net_128", "one_hidden", "three_hidden"]
KEY = prng.prng_key(11)


def _first_step(ctx, dev, c, scheme, label, prof=False, kinks=False):
    new_key_e, e1, e2 = sac.sample_noise(KEY, c.B, c.A, bool(scheme))
    new, met, grads, aux = c.twin(c.state, (e1, e2))
    r = Run(ctx, dev, c, c.state, KEY, scheme, prof=prof)
    assert np.array_equal(r.key, new_key_e) and r.count == 1          # the oracle's keys[0]; opt_count advances by one
    if kinks:
        grads = (grads[0], admissible_critic_gradient(c, r, grads[1], aux, label), grads[2])
    check_first_step(r, new, met, grads, label)
    return r, new, (e1, e2)


@pytest.mark.parametrize("scheme", [1, 0])
@pytest.mark.parametrize("name", SMALL)
def test_update_matches_twin_small(ctx, dev, name, scheme):
    _first_step(ctx, dev, Case(*CASES[name]), scheme, f"{name} scheme={scheme}")


def test_update_matches_twin_defaults_and_second_step(ctx, dev):
    """obs 376 / act 17 / hidden 256 / batch 256; then a second step from the twin's state after the first: non-zero moments in
    all three optimisers, count 1"""
    c = Case(*CASES["defaults"])
    r, new, _ = _first_step(ctx, dev, c, 1, "defaults")
    assert np.array_equal(Run(ctx, dev, c, c.state, KEY, 1).out["Q"], r.out["Q"])
    st1 = {k: (np.asarray(v, np.float32).astype(np.float64) if k != "count" else v) for k, v in new.items()}
    assert st1["count"] == 1 and all(np.any(st1[k] != 0) for k in ("pm", "pv", "qm", "qv", "am", "av"))
    key2 = prng.prng_key(12)
    _, e1, e2 = sac.sample_noise(key2, c.B, c.A, True)
    new2, _, _, _ = c.twin(st1, (e1, e2))
    r2 = Run(ctx, dev, c, st1, key2, 1)
    assert r2.count == 2
    check_second_step(r2, new2)


def test_update_split_operand_engine(ctx, dev):
    """4096 rows: the hidden layers take the split-operand images (engine 1) in every forward, input-gradient and weight-gradient
    launch; the critics' first layer, whose 393 input columns are no multiple of four, has no image and stays on the exact
    engine in the forward pass (trunk_images).  4096 x 512 unit-samples per critic pass: the critics' gradient is held to its bar
    on the admissible float32 set (admissible_critic_gradient)"""
    c = Case(376, 17, 4096, [256, 256], [256, 256], 2, 25, 2)
    r, _, _ = _first_step(ctx, dev, c, 1, "split-operand", prof=True, kinks=True)
    rows = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    print("tqc 4096 gemm rows:", [(q["kernel"], q["engine"], q["M"], q["N"], q["K"], q["launches"]) for q in rows])
    if ctx.get_counter("gemm_bx") != 1:
        assert all(q["engine"] == 0 for q in rows), rows
        return
    hidden = [q for q in rows if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (4096, 256, 256)]
    assert hidden and {q["engine"] for q in hidden} == {1}, hidden          # layer 2 of the policy, the critics and the targets
    pol_l1 = [q for q in rows if q["kernel"] == "k_gemm_fwd" and (q["N"], q["K"]) == (256, 376)]
    assert pol_l1 and {q["engine"] for q in pol_l1} == {1}, pol_l1
    cri_l1 = [q for q in rows if q["kernel"] == "k_gemm_fwd" and (q["N"], q["K"]) == (256, 393)]
    assert cri_l1 and {q["engine"] for q in cri_l1} == {0}, cri_l1
    back = [q for q in rows if q["kernel"] in ("k_gemm_dx", "k_gemm_dw") and 393 not in (q["M"], q["N"], q["K"])]
    assert back and {q["engine"] for q in back} == {1}, back


def test_update_with_critic_observation_columns(ctx, dev):
    """the policy reads 12 columns, the critics 9 others (hp->critic_states / critic_next_states)"""
    _first_step(ctx, dev, Case(12, 3, 70, [64, 64], [64, 64], 2, 25, 2, Oc=9), 1, "critic_states")


def test_two_identical_calls_give_identical_bits(ctx, dev):
    c = Case(*CASES["five_nets"])
    assert Run(ctx, dev, c, c.state, KEY).same_bits(Run(ctx, dev, c, c.state, KEY))


def test_injected_noise_equals_the_keyed_draw(ctx, dev):
    """rlx_dbg_set_sac_noise with the float32 values the oracle draws from the key: the update from the key itself, within the bars
    (the device's normal() and the oracle's agree to a few float32 ulps, not bit for bit)"""
    c = Case(*CASES["five_nets"])
    _, e1, e2 = sac.sample_noise(KEY, c.B, c.A, True)
    e1, e2 = e1.astype(np.float32), e2.astype(np.float32)
    new, met, grads, _ = c.twin(c.state, (e1, e2))
    keyed = Run(ctx, dev, c, c.state, KEY)
    inj = Run(ctx, dev, c, c.state, KEY, inject=(e1, e2))
    check_first_step(inj, new, met, grads, "injected")
    assert np.array_equal(inj.key, keyed.key)
    assert _rel(inj.out["pm"], keyed.out["pm"].astype(np.float64)) < 1e-5 and _rel(inj.out["qm"], keyed.out["qm"].astype(np.float64)) < 1e-5
    np.testing.assert_allclose(inj.metrics[:6], keyed.metrics[:6], rtol=1e-5, atol=1e-5)
    # other noise gives another update: the hook is read
    other = Run(ctx, dev, c, c.state, KEY, inject=(e2, e1))
    assert _rel(other.out["pm"], keyed.out["pm"].astype(np.float64)) > 1e-2


@pytest.mark.parametrize("what,code,word", [
    ("hidden96", -4, "hidden widths"), ("tanh", -1, "act = RLX_ACT_RELU"), ("ln_first", -1, "ln_first"), ("out_dim", -1, "qdesc->out_dim"),
    ("in_dim", -1, "qdesc->in_dim"), ("act65", -4, "act_dim"), ("atoms129", -4, "total atoms")])
def test_refusals_just_outside_the_envelope(ctx, dev, what, code, word):
    O, A, N, E = 8, 2, 25, 2
    ph, qh, act, ln, qin, qout = [64, 64], [64, 64], nets.ACT_RELU, False, None, None
    if what == "hidden96":
        qh = [64, 96]
    elif what == "tanh":
        act = nets.ACT_TANH
    elif what == "ln_first":
        ln = True
    elif what == "out_dim":
        qout = N + 1
    elif what == "in_dim":
        qin = A
    elif what == "act65":
        A = 65
    elif what == "atoms129":
        E, N = 3, 43
    pd = mlp_desc(O, ph, 2 * A, act, False, False)
    qd = mlp_desc(O + A if qin is None else qin, qh, N if qout is None else qout, nets.ACT_RELU, ln, False)
    hp = TqcHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, LR, 0.9, 0.999, 1e-8, 1.0, E, N, 2)
    x = torch.zeros(64, device=dev)
    with pytest.raises(RlxError) as e:
        ctx.tqc_update(pd, x, x, x, qd, x, x, x, x, x, x, x, (x, x, x, x, x), KEY, 0, hp, x)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(x).item() == 0
