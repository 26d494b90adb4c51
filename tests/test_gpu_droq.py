"""GPU: rlx_droq_update_f32 -- the whole DroQ update, G critic steps and one policy step over Dropout -> LayerNorm -> ReLU critics --
against the float64 twin (tests/droq_twin.py) on the same float32 inputs.  tests/test_gpu_redq.py's recipe, figures() and BARS: the
noise is injected through rlx_dbg_set_sac_noise, the library's target subsets (subsets_out) are fed to the twin, and so are the
dropout masks, which the twin gets from the Python restatement of the library's mask stream (droq_twin.update_masks over the oracle's
key chain; tests/test_gpu_droq_block.py holds that restatement equal to the device's, bit for bit).

ONE critic step is held to BARS unchanged.  Several critic steps, and 4096 rows, compound float32 rounding: those cases are held to
max(bar, 2 x F32_GAP), F32_GAP being the twin evaluated in numpy float32 against the twin in float64 on the same inputs, noise,
subsets and masks (measured once on a CPU: this file run as a script, repository root, tests and rl-x_amd on PYTHONPATH)."""
import numpy as np
import pytest
import torch

import droq_twin as tw
from oracle import nets, prng
from rlx_amd.hip import DroqHparams, RlxError, mlp_desc, redq_subset
from test_gpu_redq import BARS, GAMMA, LR, TAU, _rel, _t, figures, twin_metrics_vector

pytestmark = pytest.mark.gpu

KEY = prng.prng_key(11)

#         O  A   B   policy hidden critic hidden   E  M  G  Oc    lr_critic_delta rate
CASES = {
    "g1": (5, 2, 67, [64, 64], [64, 64], 2, 2, 1, None, 0.0, 0.25),
    "g3": (5, 2, 67, [64, 64], [64, 64], 2, 2, 3, None, -2e-5, 0.25),
    "rate001": (5, 2, 67, [64, 64], [64, 64], 2, 2, 2, None, 0.0, 0.01),
    "rate0": (5, 2, 67, [64, 64], [64, 64], 2, 2, 2, None, 0.0, 0.0),
    "e3m2": (5, 2, 67, [64, 64], [64, 64], 3, 2, 2, None, 0.0, 0.25),
    "one_net": (5, 2, 67, [64, 64], [64, 64], 1, 1, 2, None, 0.0, 0.25),
    "critic_states": (12, 3, 70, [64, 64], [64, 64], 2, 2, 2, 9, 0.0, 0.25),
    "one_layer": (5, 2, 67, [64, 64], [128], 2, 2, 2, None, 0.0, 0.25),
    "three_layers": (5, 2, 67, [64, 64], [64, 192, 128], 2, 2, 2, None, 0.0, 0.25),
    "rows4096": (5, 2, 4096, [64, 64], [64, 64], 2, 2, 2, None, 0.0, 0.25),
}
# figures() of the twin in numpy float32 against the twin in float64 (G > 1 and 4096 rows only); a figure missing here is below a
# tenth of its one-step bar: over the nine cases metrics <= 3.0e-7, norms <= 3.3e-7, pm / qm <= 3.3e-7, la 9.8e-9, P99 / Q99 <= 8.1e-8,
# Pmax / Qmax <= 2.2e-6 (bar 6.0e-4), QT below its relative part.  The second moments' 1.3e-5 is float32's 1 - 0.999, the same in
# every float32 Adam (test_gpu_redq.py).  Twice every gap is below its one-step bar: these cases meet the one-step bars.
F32_GAP = {
    "g3": {"pv": 1.27e-05, "qv": 1.29e-05},
    "rate001": {"pv": 1.29e-05, "qv": 1.28e-05},
    "rate0": {"pv": 1.29e-05, "qv": 1.29e-05},
    "e3m2": {"pv": 1.29e-05, "qv": 1.29e-05},
    "one_net": {"pv": 1.30e-05, "qv": 1.29e-05},
    "critic_states": {"pv": 1.28e-05, "qv": 1.30e-05},
    "one_layer": {"pv": 1.29e-05, "qv": 1.28e-05},
    "three_layers": {"pv": 1.29e-05, "qv": 1.32e-05},
    "rows4096": {"pv": 1.32e-05, "qv": 1.30e-05},
}


class Case:
    """name: a key of CASES -- or a row in CASES' form for a case of another table (tests/ens_cases.py), then called `label`, drawn from
    `seed` (the inputs) and seed + 1 (the noise), with no float32 gap until that table sets one (self.gap)"""

    def __init__(self, name, label=None, seed=None):
        O, A, B, ph, qh, E, M, G, Oc, delta, rate = CASES[name] if isinstance(name, str) else name
        name = name if isinstance(name, str) else label
        self.name, self.O, self.A, self.B, self.E, self.M, self.G, self.Oc, self.delta = name, O, A, B, E, M, G, O if Oc is None else Oc, delta
        self.rate, self.qh = rate, qh
        self.gap = F32_GAP.get(name, {})
        p = tw.problem(O + B + G if seed is None else seed, O, A, B, ph, qh, E, M, G, Oc, rate=rate)
        self.ps, self.qs, self.state, self.batch, self.cbatch, self.h = p["ps"], p["qs"], p["state"], p["batch"], p["cbatch"], p["h"]
        rng = np.random.default_rng(7 + B if seed is None else seed + 1)
        self.eps = (rng.standard_normal((G, B, A)).astype(np.float32), rng.standard_normal((B, A)).astype(np.float32))
        self.pd = mlp_desc(O, ph, 2 * A, nets.ACT_RELU, False, False)
        self.qd = mlp_desc(self.Oc + A, qh, 1, nets.ACT_RELU, False, False)

    def hp(self):
        hp = DroqHparams(GAMMA, TAU, self.h["target_entropy"], -20.0, 2.0, LR, LR, self.delta, LR, 0.9, 0.999, 1e-8, self.E, self.M, self.G)
        hp.dropout_rate = self.rate
        return hp

    def chain(self, key, scheme):
        """the oracle's key chain (droq.py:229-230, :247-248): G splits of 3 B + 2, one of 2 B + 1 -> (returned key, the G sample keys,
        the key each step splits)"""
        part, sks, step_keys = bool(scheme), [], []
        key = np.asarray(key, np.uint32)
        for _ in range(self.G):
            step_keys.append(key)
            ks = prng.split(key, 3 * self.B + 2, part)
            key, sk = ks[0], ks[1]
            sks.append(sk)
        step_keys.append(key)
        return prng.split(key, 2 * self.B + 1, part)[0], sks, step_keys

    def subsets(self, key, scheme):
        return np.array([prng.permutation_rows(sk, np.arange(self.E)[None], bool(scheme))[0, :self.M] for sk in self.chain(key, scheme)[1]])

    def masks(self, key, scheme):
        return tw.update_masks(self.chain(key, scheme)[2], self.B, self.qh, self.E, self.M, self.rate, bool(scheme), fast=True)

    def twin(self, st, eps, subsets, masks, dtype=np.float64):
        cb = self.cbatch or (None, None)
        st = {k: (np.asarray(v, np.float32).astype(dtype) if k in tw.STATE_KEYS else v) for k, v in st.items()}
        return tw.update(self.ps, self.qs, st, self.batch, eps[0], eps[1], subsets, masks, self.h, LR, LR, self.delta, LR, TAU, cb[0], cb[1])


class Run:
    """one rlx_droq_update_f32 call on device copies of a twin state"""

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
            self.key, self.q_count, self.pi_count, self.subsets = ctx.droq_update(
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


def f32_gap(c):
    """the twin in numpy float32 against the twin in float64 (the subsets and masks are the oracle's for KEY)"""
    sub, masks = c.subsets(KEY, 1), c.masks(KEY, 1)
    new, met, _, _ = c.twin(c.state, c.eps, sub, masks)
    new32, met32, _, _ = c.twin(c.state, c.eps, sub, masks, np.float32)
    return figures(new32, twin_metrics_vector(met32), new, met)


def bars_of(c):
    return {k: max(b, 2 * c.gap.get(k, 0.0)) for k, b in BARS.items()}


def check(c, r, new, met, label):
    f, bars = figures(r.out, r.metrics, new, met), bars_of(c)
    print(f"droq update {label}: " + " ".join(f"{k} {v:.2e}/{bars[k]:.1e}" for k, v in f.items()))
    assert r.metrics[9] == 0.0
    bad = {k: (v, bars[k]) for k, v in f.items() if not v <= bars[k]}
    assert not bad, bad


def _run_and_check(ctx, dev, name, scheme=1, prof=False):
    c = name if isinstance(name, Case) else Case(name)                             # (a Case of another table: tests/ens_cases.py)
    name = c.name
    r = Run(ctx, dev, c, c.state, KEY, scheme, inject=c.eps, prof=prof)
    key_e, sks, _ = c.chain(KEY, scheme)
    assert np.array_equal(r.key, key_e)                                            # the oracle's chain: G splits of 3 B + 2, one of 2 B + 1
    assert (r.q_count, r.pi_count) == (c.G, 1)
    assert r.subsets.shape == (c.G, c.M)
    for i, sk in enumerate(sks):
        assert np.array_equal(r.subsets[i], redq_subset(sk, c.E, c.M, scheme)), i
    assert np.array_equal(r.subsets, c.subsets(KEY, scheme))
    new, met, g, ys = c.twin(c.state, c.eps, r.subsets, c.masks(KEY, scheme))
    check(c, r, new, met, f"{name} scheme={scheme}")
    return c, r, new, met, g


@pytest.mark.parametrize("scheme", [1, 0])
def test_one_critic_step_matches_twin(ctx, dev, scheme):
    """O 5, A 2, B 67, hidden [64, 64], E 2, M 2, rate 0.25, G 1: BARS unchanged"""
    assert "g1" not in F32_GAP
    c, r, _, _, _ = _run_and_check(ctx, dev, "g1", scheme)
    m = c.masks(KEY, scheme)
    assert all(0.1 < (~x).mean() < 0.4 for part in (m["online"][0], m["target"][0], m["policy"]) for net in part for x in net)


@pytest.mark.parametrize("name", ["g3", "rate001", "rate0", "e3m2", "one_net", "critic_states", "one_layer", "three_layers"])
def test_several_critic_steps_match_twin(ctx, dev, name):
    """G 3 with a moving critic learning rate; rate 0.01 and 0; E 3 / M 2: the target pass uses parts 0 and 1 of a 3-way split; E 1;
    the critics' own observation columns (Oc 9 != O 12); one hidden layer; three unequal hidden layers"""
    c, r, new, met, g = _run_and_check(ctx, dev, name)
    norms = [np.linalg.norm(x) for x in g["gq"]]
    assert r.metrics[7] == pytest.approx(np.mean(norms), rel=1e-5)
    assert r.metrics[0] == pytest.approx(float(met["loss/q_loss"]), rel=1e-5, abs=1e-5)
    # Adam and Polyak ran over the LayerNorm parameters too
    L0 = c.qs.layers[0]
    ln = slice(L0["g"], L0["be"] + L0["out"])
    assert np.all(r.out["Q"][ln] != c.state["Q"][ln].astype(np.float32)) and np.any(r.out["QT"][ln] != c.state["QT"][ln].astype(np.float32))


def test_second_call_from_nonzero_moments_and_counts(ctx, dev):
    """a second call from the twin's state after the first: non-zero moments in all three optimisers, counters (3, 1) -> (6, 2)"""
    c = Case("g3")
    new, _, _, _ = c.twin(c.state, c.eps, c.subsets(KEY, 1), c.masks(KEY, 1))
    st1 = {k: (np.asarray(v, np.float32).astype(np.float64) if k in tw.STATE_KEYS else v) for k, v in new.items()}
    assert (st1["q_count"], st1["pi_count"]) == (3, 1) and all(np.any(st1[k] != 0) for k in ("pm", "pv", "qm", "qv", "am", "av"))
    key2 = prng.prng_key(12)
    r2 = Run(ctx, dev, c, st1, key2, 1, inject=c.eps)
    assert (r2.q_count, r2.pi_count) == (6, 2)
    new2, met2, _, _ = c.twin(st1, c.eps, r2.subsets, c.masks(key2, 1))
    check(c, r2, new2, met2, "g3, second call")


def test_rows_4096_split_operand_engine_and_image_rebuild(ctx, dev):
    """4096 rows: the hidden layers take the split-operand images, rebuilt in front of every critic step; test_gpu_redq.py's
    profiler-row counts for engine 1: per critic step policy 1, targets M, online E; policy step: policy 1, online E"""
    c, r, _, _, _ = _run_and_check(ctx, dev, "rows4096", prof=True)
    rows = [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")]
    print("droq 4096 gemm rows:", [(q["kernel"], q["engine"], q["M"], q["N"], q["K"], q["launches"]) for q in rows])
    if ctx.get_counter("gemm_bx") != 1:
        assert all(q["engine"] == 0 for q in rows), rows
        return
    hidden = [q for q in rows if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (4096, 64, 64)]
    assert hidden and {q["engine"] for q in hidden} == {1} and sum(q["launches"] for q in hidden) == c.G * (1 + c.M + c.E) + 1 + c.E, hidden
    first = [q for q in rows if q["kernel"] == "k_gemm_fwd" and q["K"] in (5, 7)]
    assert first and {q["engine"] for q in first} == {0}, first


def test_two_identical_calls_give_identical_bits(ctx, dev):
    for name in ("g3", "rows4096"):
        c = Case(name)
        assert Run(ctx, dev, c, c.state, KEY).same_bits(Run(ctx, dev, c, c.state, KEY)), name
        assert Run(ctx, dev, c, c.state, KEY, inject=c.eps).same_bits(Run(ctx, dev, c, c.state, KEY, inject=c.eps)), name


@pytest.mark.parametrize("scheme", [1, 0])
def test_keyed_noise_equals_the_oracle_draw(ctx, dev, scheme):
    """without the hook the noise comes from the keys: row b of critic step i draws normal(split(key_i, 3 B + 2)[2 + 3 b], (A,)), row
    b of the policy step normal(split(key_G, 2 B + 1)[1 + 2 b], (A,)).  The keyed run meets the bars against the twin on the oracle's
    draws, and equals the run they are injected into (test_gpu_redq.py's check)"""
    c = Case("g3")
    part = bool(scheme)
    _, _, step_keys = c.chain(KEY, scheme)
    e1 = np.stack([np.stack([prng.normal(k, (c.A,), part) for k in prng.split(step_keys[i], 3 * c.B + 2, part)[2::3]]) for i in range(c.G)])
    e2 = np.stack([prng.normal(k, (c.A,), part) for k in prng.split(step_keys[c.G], 2 * c.B + 1, part)[1::2]])
    assert e1.shape == (c.G, c.B, c.A) and e2.shape == (c.B, c.A)
    keyed = Run(ctx, dev, c, c.state, KEY, scheme)
    new, met, _, _ = c.twin(c.state, (e1, e2), keyed.subsets, c.masks(KEY, scheme))
    check(c, keyed, new, met, f"keyed scheme={scheme}")
    inj = Run(ctx, dev, c, c.state, KEY, scheme, inject=(e1, e2))
    assert np.array_equal(inj.key, keyed.key) and np.array_equal(inj.subsets, keyed.subsets)
    assert _rel(inj.out["pm"], keyed.out["pm"].astype(np.float64)) < 1e-5 and _rel(inj.out["qm"], keyed.out["qm"].astype(np.float64)) < 1e-5
    other = Run(ctx, dev, c, c.state, KEY, scheme, inject=(e1[::-1].copy(), e2))
    assert _rel(other.out["qm"], keyed.out["qm"].astype(np.float64)) > 1e-3


def test_swapped_dropout_layouts_miss_the_bars(ctx, dev):
    """the masks are read, each from its own key layout: the twin fed the online and target masks EXCHANGED (what reading
    keys[4 + 3 b] for the online critics and keys[3 + 3 b] for the targets would give) is far outside the bars of the same run"""
    c = Case("g1")
    r = Run(ctx, dev, c, c.state, KEY, 1, inject=c.eps)
    masks = c.masks(KEY, 1)
    new, met, _, _ = c.twin(c.state, c.eps, r.subsets, masks)
    check(c, r, new, met, "g1 (own masks)")
    news, mets, _, _ = c.twin(c.state, c.eps, r.subsets, tw.swap_online_target(masks, c.M))
    f, bars = figures(r.out, r.metrics, news, mets), bars_of(c)
    print("droq update g1 against swapped masks: " + " ".join(f"{k} {v:.2e}/{bars[k]:.1e}" for k, v in f.items()))
    assert f["qm"] > 100 * bars["qm"] and f["metrics"] > 100 * bars["metrics"]
    # and all-ones masks (no dropout at all) miss them too
    ones = {k: ([[[np.ones_like(x) for x in net] for net in step] for step in v] if k != "policy" else [[np.ones_like(x) for x in net] for net in v])
            for k, v in masks.items()}
    newo, meto, _, _ = c.twin(dict(c.state), c.eps, r.subsets, ones)
    assert figures(r.out, r.metrics, newo, meto)["qm"] > 100 * bars["qm"]


@pytest.mark.parametrize("what,code,word", [
    ("rate_one", -1, "dropout_rate"), ("rate_negative", -1, "dropout_rate"), ("hidden_832", -4, "768"), ("e17", -4, "ensemble_size"),
    ("g0", -1, "q_update_steps"), ("m_above_e", -1, "in_target_minimization_size"), ("one_critic_pointer", -1, "critic_states")])
def test_refusals_leave_the_outputs_alone(ctx, dev, what, code, word):
    O, A, E, M, G, rate, qh = 8, 2, 2, 2, 2, 0.01, [64, 64]
    if what == "rate_one":
        rate = 1.0
    elif what == "rate_negative":
        rate = -0.01
    elif what == "hidden_832":
        qh = [64, 832]
    elif what == "e17":
        E = 17
    elif what == "g0":
        G = 0
    elif what == "m_above_e":
        M = 3
    pd = mlp_desc(O, [64, 64], 2 * A, nets.ACT_RELU, False, False)
    qd = mlp_desc(O + A, qh, 1, nets.ACT_RELU, False, False)
    hp = DroqHparams(GAMMA, TAU, -1.0, -20.0, 2.0, LR, LR, 0.0, LR, 0.9, 0.999, 1e-8, E, M, G)
    hp.dropout_rate = rate
    x = torch.zeros(64, device=dev)
    if what == "one_critic_pointer":
        hp.critic_states = x.data_ptr()
    with pytest.raises(RlxError) as e:
        ctx.droq_update(pd, x, x, x, qd, x, x, x, x, x, x, x, (x, x, x, x, x), KEY, 0, 0, hp, x)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(x).item() == 0


if __name__ == "__main__":      # the float32 gaps behind F32_GAP (CPU only)
    for name in CASES:
        if name == "g1":
            continue
        gap = f32_gap(Case(name))
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in gap.items() if v > 0.1 * BARS[k]) + "},")
        print("      # all:", " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
