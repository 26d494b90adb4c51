"""GPU: rlx_td3_update_f32 -- TD3's critic step with or without the policy step, and DDPG's joint step -- against the float64 twin
(tests/td3_twin.py) on the same float32 inputs, with the smoothing noise injected through rlx_dbg_set_sac_noise.

Cases and figures: tests/td3_cases.py.  Bars for ONE call (BARS) are tests/test_gpu_redq.py's, restated: metrics 1e-5 relative and
absolute, the two norms 1e-5 relative; first moments (a first step's are gradients / 10) 1e-5 relative L2; second moments 5e-5
relative L2 (float32's 1 - 0.999 is 1.29e-5 off 0.001, in every float32 Adam); parameter steps within 2e-5 on 99 % of the entries and
within 2 lr + 1e-6 everywhere; targets rtol 1e-4, atol 2 lr tau + 1e-6 -- the policy's target under the critics' bar.

Two calls in a row, and 4096 rows, compound float32 rounding: the twin evaluated in numpy float32 on the same inputs is itself off
the float64 twin by F32_GAP below (measured once on a CPU: this file run as a script, repository root and rl-x_amd on PYTHONPATH).
Those cases are held to twice that gap or to the one-call bar, whichever is larger."""
import numpy as np
import pytest
import torch

import td3_cases as tc
import td3_twin as tw
from oracle import nets, prng
from rlx_amd.hip import RlxError, Td3Hparams, mlp_desc

pytestmark = pytest.mark.gpu

GAMMA, TAU, LR = tc.GAMMA, tc.TAU, tc.LR
KEY = prng.prng_key(11)

BARS = {"metrics": 1e-5, "norms": 1e-5, "pm": 1e-5, "qm": 1e-5, "pv": 5e-5, "qv": 5e-5, "P99": 2e-5, "Q99": 2e-5,
        "Pmax": 2 * LR + 1e-6, "Qmax": 2 * LR + 1e-6, "QT": 2 * LR * TAU + 1e-6, "PT": 2 * LR * TAU + 1e-6}

# figures() of the twin in numpy float32 against the twin in float64, same inputs and noise (tc.COMPOUNDING only).  Measured on a CPU;
# a figure missing here is below a tenth of its one-call bar: over the two cases metrics <= 8.8e-8, norms <= 2.0e-7, pm / qm <= 4.7e-7,
# P99 / Q99 <= 2.3e-8, Pmax / Qmax <= 5.5e-7, QT / PT below their relative part.  The second moments' 1.3e-5 is float32's 1 - 0.999
# (above), the same in every case.  Twice every gap is below its one-call bar: these cases meet the one-call bars.
F32_GAP = {
    "two_calls": {"pv": 1.29e-05, "qv": 1.30e-05},
    "split_ragged": {"pv": 1.28e-05, "qv": 1.33e-05},
}


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def hparams(c, pstep=True, lrp=LR, lrq=LR):
    return Td3Hparams(GAMMA, TAU, c.h["smoothing_epsilon"], c.h["smoothing_clip_value"], lrp, lrq, 0.9, 0.999, 1e-8, c.E, int(c.joint),
                      int(pstep))


class Run:
    """one rlx_td3_update_f32 call on device copies of a twin state"""

    def __init__(self, ctx, dev, c, st, key, call=(True, LR, LR), scheme=1, inject=None, prof=False):
        self.t = {k: _t(st[k], dev) for k in tw.STATE_KEYS}
        t = self.t
        met = torch.full((5,), 7.0, device=dev)
        hp = hparams(c, *call)
        keep = [_t(x, dev) for x in c.cbatch] if c.cbatch else []
        if keep:
            hp.critic_states, hp.critic_next_states = keep[0].data_ptr(), keep[1].data_ptr()
        eps = None if inject is None else _t(inject, dev)                  # kept alive: the library holds the pointer
        pd, qd = c.descs()
        if eps is not None:
            ctx.dbg_set_sac_noise(eps, None)
        if prof:
            ctx.prof_begin()
        try:
            self.key, self.q_count, self.pi_count = ctx.td3_update(
                pd, t["P"], t["pm"], t["pv"], t["PT"], qd, t["Q"], t["qm"], t["qv"], t["QT"], tuple(_t(x, dev) for x in c.batch),
                np.asarray(key, np.uint32), st["q_count"], st["pi_count"], hp, met, scheme)
        finally:
            ctx.dbg_set_sac_noise(None, None)
            if prof:
                ctx.prof_end()
        torch.cuda.synchronize()
        self.out = {k: v.cpu().numpy() for k, v in t.items()}
        self.out.update(q_count=self.q_count, pi_count=self.pi_count)
        self.metrics = met.cpu().numpy()

    def same_bits(self, other):
        return all(np.array_equal(self.out[k], other.out[k]) for k in tw.STATE_KEYS) and np.array_equal(self.metrics, other.metrics) \
            and np.array_equal(self.key, other.key)


def check(c, r, new, met, old, label):
    f = tc.figures(r.out, r.metrics, new, met, old)
    gap = F32_GAP.get(c.name, {})
    bars = {k: max(BARS[k], 2 * gap.get(k, 0.0)) for k in f}
    print(f"td3 update {label}: " + " ".join(f"{k} {v:.2e}/{bars[k]:.1e}" for k, v in f.items()))
    bad = {k: (v, bars[k]) for k, v in f.items() if not v <= bars[k]}
    assert not bad, bad


def _run_and_check(ctx, dev, name, scheme=1, prof=False):
    c = tc.Case(name)
    assert len(c.calls) == 1
    r = Run(ctx, dev, c, c.state, KEY, c.calls[0], scheme, inject=c.eps, prof=prof)
    new, met, aux = c.twin()[0]
    # the oracle's chain: one split of B + 1 (td3.py:149-150); DDPG's update takes no key
    assert np.array_equal(r.key, KEY if c.joint else prng.split(KEY, c.B + 1, bool(scheme))[0])
    assert (r.q_count, r.pi_count) == (new["q_count"], new["pi_count"])
    check(c, r, new, met, c.state, f"{name} scheme={scheme}")
    return c, r, new, met


def test_critic_step_only_leaves_targets_and_policy_alone(ctx, dev):
    c, r, new, met = _run_and_check(ctx, dev, "critic_only")
    assert (r.q_count, r.pi_count) == (1, 0)
    for k in ("P", "pm", "pv", "PT", "QT"):                              # bit-unchanged
        assert np.array_equal(r.out[k], np.asarray(c.state[k], np.float32)), k
    assert np.array_equal(r.metrics[2:], np.full(3, 7.0, np.float32))     # the policy step's metrics are left alone


@pytest.mark.parametrize("scheme", [1, 0])
def test_critic_and_policy_step_match_twin(ctx, dev, scheme):
    """O 5, A 2, B 67, hidden [64, 64]: the full TD3 update under both key schemes"""
    c, r, new, met = _run_and_check(ctx, dev, "full", scheme)
    assert (r.q_count, r.pi_count) == (1, 1)
    for k in ("QT", "PT"):                                                # the targets moved
        assert not np.array_equal(r.out[k], np.asarray(c.state[k], np.float32)), k


def test_ddpg_joint_step_matches_twin(ctx, dev):
    c, r, new, met = _run_and_check(ctx, dev, "ddpg")
    assert (r.q_count, r.pi_count) == (1, 1)
    # TD3's order on the same inputs (the policy step against the STEPPED critic) is another policy gradient: the bars see the difference
    st64 = tw.cast_state(c.state, np.float64)
    after, _, _ = tw.critic_step(c.ps, c.qs, st64, c.batch, None, c.h, LR)
    _, gp_td3, _ = tw.policy_grads(c.ps, c.qs, st64["P"], after["Q"], np.asarray(c.batch[0], np.float64), c.h)
    assert tc._rel(gp_td3 / 10.0, new["pm"]) > 10 * BARS["pm"]


def test_second_call_unequal_counts_and_annealed_rates(ctx, dev):
    """two calls in a row: a critic-only call (counts 0, 0 -> 1, 0), then a full call at annealed, unequal rates from the non-zero
    critic moments the first left (1, 0 -> 2, 1): the critics' Adam step is its second, the policy's its first"""
    c = tc.Case("two_calls")
    r1 = Run(ctx, dev, c, c.state, KEY, c.calls[0], inject=c.eps)
    assert (r1.q_count, r1.pi_count) == (1, 0) and np.any(r1.out["qm"] != 0)
    r2 = Run(ctx, dev, c, r1.out, r1.key, c.calls[1], inject=c.eps)
    assert (r2.q_count, r2.pi_count) == (2, 1)
    (n1, m1, _), (n2, m2, _) = c.twin()
    assert np.array_equal(r2.key, prng.split(prng.split(KEY, c.B + 1)[0], c.B + 1)[0])
    check(c, r2, n2, m2, n1, "two_calls, second call")
    # equal rates and counts would read differently: the first moments' bias correction at count 1 vs 2 alone is 1 - 0.9 vs 1 - 0.81
    same = c.twin_call(n1, (True, LR, LR))[0]
    assert np.abs(same["Q"] - n2["Q"]).max() > 2 * BARS["Q99"]


@pytest.mark.parametrize("name", ["critic_states", "narrow", "act64"])
def test_shapes_match_twin(ctx, dev, name):
    _run_and_check(ctx, dev, name)


def test_split_ragged_rows_4099(ctx, dev):
    """4099 rows: the hidden layers take the split-operand images (rebuilt in front of the policy step from the stepped critics: stale
    images would evaluate it with the old ones), three rows past the last full tile"""
    c, r, _, _ = _run_and_check(ctx, dev, "split_ragged", prof=True)
    rows = [q for q in ctx.prof_rows() if q["kernel"] == "k_gemm_fwd" and q["M"] == c.B]
    print("td3 4099 forward gemm rows:", [(q["engine"], q["N"], q["K"], q["launches"]) for q in rows])
    if ctx.get_counter("gemm_bx") == 1:
        hidden = [q for q in rows if (q["N"], q["K"]) == (128, 256)]
        # critic step: target policy 1, targets 2, online 2; policy step: policy 1, online 2
        assert hidden and {q["engine"] for q in hidden} == {1} and sum(q["launches"] for q in hidden) == 8, hidden


def test_two_identical_calls_give_identical_bits(ctx, dev):
    for name in ("full", "ddpg", "split_ragged"):
        c = tc.Case(name)
        assert Run(ctx, dev, c, c.state, KEY).same_bits(Run(ctx, dev, c, c.state, KEY)), name
        if c.eps is not None:
            assert Run(ctx, dev, c, c.state, KEY, inject=c.eps).same_bits(Run(ctx, dev, c, c.state, KEY, inject=c.eps)), name


@pytest.mark.parametrize("scheme", [1, 0])
def test_keyed_noise_equals_the_oracle_draw(ctx, dev, scheme):
    """without the hook row b draws normal(split(key, B + 1)[1 + b], (A,)).  The device's normal() and the oracle's agree to a few
    float32 ulps, not bit for bit: the keyed run meets the bars against the twin on the oracle's draws and equals the run they are
    injected into; with the oracle's draw of row 0, 1 or B - 1 replaced, the injected run is another update"""
    c = tc.Case("full")
    rows = (0, 1, c.B - 1)
    term = c.batch[4].copy()
    term[list(rows)] = 0.0                                                 # (a terminated row's target does not read its noise)
    c.batch = c.batch[:4] + (term,)
    key_e, noise = tw.smoothing_noise(KEY, c.B, c.A, bool(scheme))
    for b in rows:
        assert np.array_equal(noise[b], prng.normal(prng.split(KEY, c.B + 1, bool(scheme))[1 + b], (c.A,), bool(scheme)))
    c.eps = noise
    keyed = Run(ctx, dev, c, c.state, KEY, scheme=scheme)
    assert np.array_equal(keyed.key, key_e)
    new, met, _ = c.twin()[0]
    check(c, keyed, new, met, c.state, f"keyed scheme={scheme}")
    inj = Run(ctx, dev, c, c.state, KEY, scheme=scheme, inject=noise)
    ref = keyed.out["qm"].astype(np.float64)
    assert tc._rel(inj.out["qm"], ref) < 1e-5
    # The margin: on the float64 twin, replacing ONE of these rows' draws moves qm by 1.4e-3 (row 0, scheme 1) ... 6.3e-3 relative,
    # 140 times the 1e-5 bar the keyed run has just met: a wrong key in any of the three rows would have put it past that bar.
    shifts = {}
    for b in rows:
        other = noise.copy()
        other[b] = -noise[b] + 0.25
        o = Run(ctx, dev, c, c.state, KEY, scheme=scheme, inject=other)
        shifts[b] = tc._rel(o.out["qm"], ref)
    print(f"td3 keyed scheme={scheme}: qm shift per replaced row " + " ".join(f"{b}: {v:.2e}" for b, v in shifts.items()))
    assert min(shifts.values()) > 1e-4, shifts


@pytest.mark.parametrize("what,code,word", [
    ("four_hidden", -1, "1..3 hidden layers"), ("width_96", -4, "multiples of 64"), ("width_1088", -4, "at most 1024"),
    ("act_65", -4, "act_dim"), ("world_2", -4, "data-parallel"),
    ("three_critics", -4, "nr_critics"), ("joint_two_critics", -1, "joint"), ("joint_smoothing", -1, "joint"),
    ("joint_no_policy_step", -1, "policy_step"), ("out_dim", -1, "qdesc->out_dim"), ("one_critic_pointer", -1, "critic_states")])
def test_refusals_leave_the_outputs_alone(ctx, dev, what, code, word):
    O, A, E, joint, smooth, pstep, qout, ph, qh = 8, 2, 2, 0, 0.2, 1, 1, [64, 64], [64, 64]
    if what == "four_hidden":
        ph = [64, 64, 64, 64]
    elif what == "width_96":
        qh = [64, 96]
    elif what == "width_1088":
        ph = [1088, 64]
    elif what == "act_65":
        A = 65
    elif what == "three_critics":
        E = 3
    elif what == "joint_two_critics":
        joint, smooth = 1, 0.0
    elif what == "joint_smoothing":
        E, joint = 1, 1
    elif what == "joint_no_policy_step":
        E, joint, smooth, pstep = 1, 1, 0.0, 0
    elif what == "out_dim":
        qout = 2
    pd = mlp_desc(O, ph, A, nets.ACT_RELU, False, False)
    qd = mlp_desc(O + A, qh, qout, nets.ACT_RELU, False, False)
    hp = Td3Hparams(GAMMA, TAU, smooth, 0.5, LR, LR, 0.9, 0.999, 1e-8, E, joint, pstep)
    x = torch.zeros(64, device=dev)
    if what == "one_critic_pointer":
        hp.critic_states = x.data_ptr()
    if what == "world_2":
        ctx.set_rank(0, 2)                                                 # (the test hook: a context of world size 2 without a communicator)
    try:
        with pytest.raises(RlxError) as e:
            ctx.td3_update(pd, x, x, x, x, qd, x, x, x, x, (x, x, x, x, x), KEY, 0, 0, hp, x)
    finally:
        ctx.set_rank(0, 1)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(x).item() == 0


def test_losses_entry_matches_twin_and_repeats_bits(ctx, dev):
    """rlx_td3_losses_f32 on given values, E = 2 and 1, B past one workgroup: y, d loss / d q and the loss"""
    rng = np.random.default_rng(3)
    for E, B in ((2, 67), (1, 67), (2, 1031)):
        q, qn = rng.standard_normal((E, B)).astype(np.float32), rng.standard_normal((E, B)).astype(np.float32)
        r, term = rng.standard_normal(B).astype(np.float32), (rng.random(B) < 0.3).astype(np.float32)
        y, loss, dq = tw.critic_loss(q.T.astype(np.float64), qn.T.astype(np.float64), r.astype(np.float64), term.astype(np.float64), GAMMA)
        hp = Td3Hparams(GAMMA, TAU, 0.2, 0.5, LR, LR, 0.9, 0.999, 1e-8, E, 0, 1)
        outs = []
        for _ in range(2):
            y_d, dq_d, l_d = torch.zeros(B, device=dev), torch.zeros(E, B, device=dev), torch.zeros(1, device=dev)
            ctx.td3_losses(_t(q, dev), _t(qn, dev), _t(r, dev), _t(term, dev), hp, dq_d, l_d, y_d)
            torch.cuda.synchronize()
            outs.append((y_d.cpu().numpy(), dq_d.cpu().numpy(), l_d.cpu().numpy()))
        assert all(np.array_equal(a, b) for a, b in zip(*outs))
        assert np.allclose(outs[0][0], y, rtol=1e-6, atol=1e-6) and np.allclose(outs[0][1], dq.T, rtol=1e-5, atol=1e-7 / B)
        assert outs[0][2][0] == pytest.approx(loss.mean(), rel=1e-6)


if __name__ == "__main__":      # the float32 gaps behind F32_GAP (CPU only)
    for name in tc.COMPOUNDING:
        gap = tc.f32_gap(tc.Case(name))
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in gap.items() if v > 0.1 * BARS[k]) + "},")
        print("      # all:", " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
