"""CPU: the conditions the shape cases of the fused acting step (rollout_cases.py, run on the device by
test_gpu_rollout_shapes.py) are chosen under.  A plain float32 evaluation of every case stays within half of each bar of the
float64 oracle; each of a handful of one-line faults put into the oracle misses a bar by 10x or more; the cases that run on the
fp16 pipe keep their operands 100x inside its window; the Python mirror of rlx_ppo_rollout_step_supported agrees with the library
over a grid of descriptors; and every case takes the kernel paths it is in the table for."""
import ctypes
import itertools

import numpy as np
import pytest

import rollout_cases as rc
from net_paths import X_ALIMIT, X_WLIMIT
from oracle import nets
from rlx_amd.hip import lib as L
from rlx_amd.hip import mlp_desc


def _oracle_steps(c, scheme, env_cls=None):
    """the case's STEPS steps through the float64 oracle alone -> [(obs, eps, expected dict, env outputs)]"""
    env = c.env() if env_cls is None else c.env(env_cls)
    key, obs, out = c.key, env.obs.copy(), []
    for _ in range(rc.STEPS):
        key, eps = c.noise(key, scheme)
        exp = c.expected(obs, eps)
        step = env.step(exp["processed"].astype(np.float32))
        out.append((obs, eps, exp, step))
        obs = step[0]
    return out


@pytest.fixture(scope="module")
def steps():
    cache = {}

    def get(name, scheme=1):
        if (name, scheme) not in cache:
            c = rc.Case(name)
            cache[(name, scheme)] = (c, _oracle_steps(c, scheme))
        return cache[(name, scheme)]
    return get


@pytest.mark.parametrize("name", rc.NAMES)
def test_a_float32_evaluation_uses_at_most_half_of_each_bar(name, steps):
    """the same float32 parameters, observations, draws and bounds the device sees, through oracle.ppo.get_action_and_value in
    float32 numpy, against the float64 evaluation: at most half of the value, action, processed-action and log-prob bars"""
    for scheme in rc.Case(name).schemes:
        c, st = steps(name, scheme)
        worst = {}
        for obs, eps, exp, _ in st:
            got = c.expected(obs, eps, dtype=np.float32)
            for k in ("value", "action", "processed", "logp"):
                worst[k] = max(worst.get(k, 0.0), rc.bar_fraction(k, got[k], exp[k]))
        print(f"{name} scheme {scheme}: float32 on the CPU, fraction of each bar: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 0.5, worst


def _zeroed(p, off, n):
    q = p.copy()
    q[off:off + n] = 0.0
    return q


def _faults(c):
    """{fault name: keyword arguments of Case.expected that put it into the oracle}"""
    ph, ch = c.ps.head, c.cs.head
    f = {
        "head without its last input row": dict(pp=_zeroed(c.pp, ph["W"] + (ph["in"] - 1) * c.A, c.A),
                                                cp=_zeroed(c.cp, ch["W"] + ch["in"] - 1, 1)),
        "last action column without its bias": dict(pp=_zeroed(c.pp, ph["b"] + c.A - 1, 1)),
    }
    if c.ps.ln_first:
        f["policy LayerNorm without its bias"] = dict(pp=_zeroed(c.pp, c.ps.layers[0]["be"], c.ps.hidden[0]))
    if c.cs.ln_first:
        f["critic LayerNorm without its bias"] = dict(cp=_zeroed(c.cp, c.cs.layers[0]["be"], c.cs.hidden[0]))
    if c.clip:
        lo, hi = c.lo.copy(), c.hi.copy()
        lo[-1], hi[-1] = c.hi[-1], c.lo[-1]
        f["lo and hi of the last action dim swapped"] = dict(lo=lo, hi=hi)
    return f


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_bars_see_one_line_faults(name, steps):
    c, st = steps(name)
    for fault, kw in _faults(c).items():
        factor = max(rc.worst_fraction(c.expected(obs, eps, **kw), exp) for obs, eps, exp, _ in st)
        print(f"{name}: {fault}: {factor:.0f}x a bar")
        assert factor >= 10.0, (fault, factor)


def test_the_reward_bar_sees_a_clamped_observation_column(steps):
    """three_valu has A > O: the env scores action dim j against obs[j % O]; with obs[min(j, O - 1)] the reward misses its bar"""
    c, st = steps("three_valu")
    assert c.A > c.O
    env = c.env(rc.ClampedColsEnv)
    factor = 0.0
    for obs, _, exp, step in st:
        env.obs = obs.copy()
        factor = max(factor, rc.bar_fraction("reward", env.step(exp["processed"].astype(np.float32))[2], step[2]))
    print(f"three_valu: obs[min(j, O - 1)]: {factor:.0f}x the reward bar")
    assert factor >= 10.0


@pytest.mark.parametrize("name", rc.NAMES)
def test_every_case_sees_finished_episodes_and_moves_its_clock(name, steps):
    c, st = steps(name)
    assert sum(int(s[3][5].sum()) for s in st) > 0
    assert rc.ENV["env_id_offset"] != 0 and c.n_global == c.N + 131 and c.N <= 70
    if c.clip:       # clipping acts: some action outside [-1, 1], and the bounds are asymmetric per dimension
        assert any(np.any(np.abs(s[2]["action"]) > 1.0) for s in st)
        assert np.all(c.lo < -0.5 + 1e-6) and np.all(c.hi > 0.5 - 1e-6) and np.unique(c.lo + c.hi).size == c.A


@pytest.mark.parametrize("name", [n for n in rc.NAMES if rc.Case(n).has_images])
def test_image_cases_stay_inside_the_fp16_window(name, steps):
    c, st = steps(name)
    w = max(float(np.abs(c.pp).max()), float(np.abs(c.cp).max()))
    trace = []
    for obs, eps, _, _ in st:
        c.expected(obs, eps, trace=trace)
    print(f"{name}: max |weight| {w:.2f}, max |hidden activation| {max(trace):.2f}")
    assert 0 < w * 100 < X_WLIMIT and 0 < max(trace) * 100 < X_ALIMIT


# ----------------------------------------------------------------------------------------------------- the support predicate
def _hidden_lists():
    h0s, later = (64, 96, 320, 512, 576), (64, 128, 192, 256, 512)
    yield ()
    for h0 in h0s:
        yield (h0,)
        for l1 in later:
            yield (h0, l1)
            for l2 in later:
                yield (h0, l1, l2)
            yield (h0, l1, l1, l1)


def test_the_mirror_of_the_support_predicate_agrees_with_the_library():
    lib = L.load_library()
    sup = lambda pd, cd: bool(lib.rlx_ppo_rollout_step_supported(ctypes.byref(pd), ctypes.byref(cd)))
    n = accepted = 0
    bad = []

    def check(p, c):
        nonlocal n, accepted
        pd, cd = mlp_desc(p[0], p[1], p[2], nets.ACT_RELU, True, p[3]), mlp_desc(c[0], c[1], c[2], nets.ACT_TANH, False, False)
        want = rc.step_supported(p[0], p[1], p[2], p[3], c[0], c[1], c[2])
        n, accepted = n + 1, accepted + int(want)
        if sup(pd, cd) != want:
            bad.append((p, c, want))
    for hidden in _hidden_lists():
        for in_dim, out_dim, logstd, c_out, match in itertools.product((0, 1, 32, 33), (0, 1, 32, 33), (True, False), (1, 2),
                                                                       (True, False)):
            c_in = in_dim if match else (1 if in_dim != 1 else 2)
            check((in_dim, hidden, out_dim, logstd), (c_in, hidden, c_out))
    # a critic of its own shape: every hidden list against one accepted policy, and the other way round
    for hidden in _hidden_lists():
        check((17, (256, 256), 6, True), (17, hidden, 1))
        check((17, hidden, 6, True), (17, (512, 256, 128), 1))
    assert not bad, bad[:10]
    assert n > 10000 and 100 < accepted < n // 4
    assert not lib.rlx_ppo_rollout_step_supported(None, None)


def test_the_head_boundary_of_the_one_layer_cases():
    """one hidden layer: the head's weights are staged into A1 | Bs (16544 floats), past the weight stage alone (8320) from
    320 x 27 on; the widest accepted head, 512 x 32 = 16384 floats, fits"""
    assert rc.RO_BS == 8320 and rc.RO_A1 + rc.RO_BS == 16544
    assert rc.head_floats((320,), 26) == rc.RO_BS and rc.head_floats((320,), 27) > rc.RO_BS
    for h0, out in itertools.product(range(64, 513, 64), range(1, 34)):
        if rc.net_supported(32, (h0,), out):
            assert rc.head_floats((h0,), out) <= rc.head_stage_floats((h0,))
        for h1 in (128, 256):
            if rc.net_supported(32, (h0, h1), out):
                assert rc.head_floats((h0, h1), out) <= rc.head_stage_floats((h0, h1)) == rc.RO_BS
    assert rc.net_supported(32, (512,), 32) and rc.head_floats((512,), 32) == 16384


# ------------------------------------------------------------------------------------------------------- per-case path claims
#        name           layer 0 (policy, critic)  LN     head floats  K into the hidden layers l >= 1 (policy)
CLAIMS = {
    "one512_a32":   (("mfma", "mfma"), True, 16384, ()),
    "one320_fit":   (("valu", "valu"), False, 8320, ()),
    "one320_over":  (("valu", "valu"), False, 8640, ()),
    "min":          (("valu", "valu"), False, 128, (64,)),
    "valu_ln_relu": (("valu", "valu"), True, 4352, (448,)),
    "mfma_noln":    (("mfma", "mfma"), False, 4096, (512, 256)),
    "mfma_two":     (("mfma", "mfma"), True, 384, (512,)),
    "three_valu":   (("valu", "valu"), True, 2304, (192, 128)),
    "mixed":        (("valu", "mfma"), False, 1536, (256,)),
}


@pytest.mark.parametrize("name", rc.NAMES)
def test_every_case_takes_the_paths_it_is_there_for(name):
    c = rc.Case(name)
    l0, ln, head, ks = CLAIMS[name]
    assert c.supported()
    assert (rc.layer0_path(c.O, c.ps.hidden), rc.layer0_path(c.O, c.cs.hidden)) == l0 and c.ps.ln_first == ln
    assert rc.head_floats(c.ps.hidden, c.A) == head <= rc.head_stage_floats(c.ps.hidden)
    assert tuple(c.ps.hidden[:-1]) == ks and c.has_images == bool(ks)
    assert c.N <= 70 and rc.NOISE_ROW_OFFSET + c.N <= c.n_global
    if name == "one512_a32":        # every per-thread slot live: 4 eps slots, 16 observation pairs, 16 MFMA k-steps
        assert c.A == rc.MAX_OUT and c.O == rc.MAX_IN and head > rc.RO_BS and len(c.ps.hidden) == 1
    if name == "one320_fit":
        assert head == rc.RO_BS
    if name == "one320_over":
        assert rc.RO_BS < head <= rc.RO_BS + 320
    if name == "min":               # the image layer runs only its peeled tail, the exact-fp32 layer one trip
        assert not rc.bx_main_loop(64) and rc.fp32_layer_trips(64) == 1 and (c.O, c.A, c.N) == (1, 1, 1)
    if name == "valu_ln_relu":
        assert c.ps.act == nets.ACT_RELU and c.O % 2 == 1 and c.ps.hidden[0] // 64 == 7 and rc.bx_main_loop(448)
    if name == "mfma_two":
        assert c.N == rc.RO_ROWS
    if name == "three_valu":
        assert c.A > c.O and c.ps.hidden[2] > c.ps.hidden[1] and c.schemes == (1, 0) and all(rc.bx_main_loop(k) for k in ks)
    if name == "mixed":
        assert c.ps.hidden != c.cs.hidden and c.ps.act != c.cs.act and c.ps.ln_first != c.cs.ln_first and c.cs.ln_first
    if name in ("one512_a32", "valu_ln_relu", "three_valu", "mixed"):
        assert c.clip
