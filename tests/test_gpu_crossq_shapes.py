"""GPU: rlx_crossq_critic_update_f32, rlx_crossq_policy_update_f32 and rlx_crossq_act_f32 (crossq.hip over brn.hip) across the shape
envelope cq_check_net, cq_check_hp and ens_prologue accept, against the float64 twin at test_gpu_crossq.py's one-step BARS (its Case,
Run, figures and check).  tests/crossq_cases.py holds the case table; nc = num_cus of the device:

| case        | O / Oc  | A  | policy hidden  | critic hidden  | E  | B           | dense_bias |
|-------------|---------|----|----------------|----------------|----|-------------|------------|
| act64       | 70 / 29 | 64 | (128, 64, 64)  | (128, 64, 64)  | 3  | 37          | 0          |
| wide_policy | 48 / 48 | 16 | (2048, 1984)   | (1984, 2048)   | 1  | 24          | 0.5        |
| half_split  | 45 / 45 | 17 | (256, 128)     | (256, 128)     | 2  | 2049        | 0          |
| e16_cut     | 8 / 9   | 3  | (64, 128, 192) | (64, 128, 192) | 16 | 4099        | 3          |
| many_rows   | 64 / 64 | 1  | (64)           | (64)           | 1  | 128 nc + 37 | 0          |
| ties        | 5 / 5   | 2  | (64, 64)       | (64, 64)       | 3  | 67          | 0          |

  act64        A 64 in both updates (four rows a block; policy head N 128), Oc 29 unaligned, Oc + A = 93 ragged, the critics' own
               observations, B odd: the joint pass has 74 rows, one slab of the column sums plus ten rows
  wide_policy  widths at the limit on the policy side; cq_dw's bands with a ragged last band (Kd 1984 into N 2048: 7 x 256 + 192) and, the
               other way round (Kd 2048 into N 1984), 4 x 512 at 4092 of REDUCE_MAX_BLOCKS' 4096 workgroups; the policy head has K 1984;
               the bias gradient comes from the first band only
  half_split   2 B = 4098 >= 4096 > B: the critics' joint pass runs on the split-operand engine, forward and backward, at M % 4 != 0,
               while the policy on s' in the same call and the whole policy update run on the exact engine; the ragged first layers
               (45, 62) stay exact while their weight gradients go split
  e16_cut      E at its limit; the image list ends INSIDE critic 5 -- at layer 2 in the critic update (3 + 5 x 5 + 1 + 2 = 31 jobs, the
               next needs 2) and at layer 1 in the policy update -- so one shape shows on both engines; the minimum and the routing of
               the gradient run over 16 critics.  Its Dense biases are raised by 3: with 0 every seed has some of the joint pass's 50 M
               pre-activations within float32 rounding of their ReLU kink, and one derivative on the other side costs up to 20 bars
               (crossq_cases.E16_DENSE_BIAS has the device's measurement and the two units it came from)
  many_rows    the joint pass has 256 nc + 74 rows: brn_rows_per_slab gives 65, BrnWalk::next runs inside the update with ld4 17 (65
               input columns: steps carry into the next row) and ld4 16 (they do not); k_crossq_critic_loss, k_crossq_policy_seed,
               ens_mean and ens_finish far past 256 rows; A 1
  ties         critic 2 is a copy of critic 0, parameters and statistics: every row in which that pair holds the minimum (33 of 67) is a
               two-way tie of k_crossq_policy_seed, whose seed there is -1 / (2 B) to each -- -1 / B to both would double dQ/da (test_crossq_cases.py
               shows the bars see that); critics 0 and 2 leave the critic update with equal bits

test_crossq_cases.py recomputes these claims from tests/net_paths.py, holds each case's float32 twin (column sums in double, as
brn.hip takes them) to half of every bar, and shows that the bars see a dropped tail row of the column sums, a zeroed last action
column and a last critic on its neighbour's parameters.

One pair of updates per case with injected noise.  The bars are the one-step bars for every case.

Measured on the MI355X (split-operand engine on), the largest figure over the six cases against its bar: metrics 4.8e-7 / 1e-5
(wide_policy), norms 9.3e-8 / 1e-5, pm 8.6e-7 / 1e-5 (wide_policy), qm 8.3e-7 / 1e-5 (wide_policy), pv 1.0e-6 / 5e-5, qv 1.1e-6 /
5e-5, ps 2.6e-8 / 1e-5, qs 2.6e-8 / 1e-5, la 1.3e-8 / 1e-6, P99 5.0e-8 / 2e-5, Q99 4.7e-8 / 2e-5, Pmax 1.0e-5 / 2e-3, Qmax 1.2e-5 /
2e-3; half_split with the engine off reads qm 2.1e-7; acting is within 1.0e-6 of 2e-6 ("Shape envelope of CrossQ and
the BRN layer", has every case)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import crossq_cases as cc
import crossq_twin as tw
import net_paths as npth
from oracle import nets
from rlx_amd.hip import RlxError, lib as L

pytestmark = pytest.mark.gpu

m = cc.m
GEMMS = ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")


def _nc():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _case(name):
    return cc.shape_case(name, _nc())


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(mid, new, met, infos) of the float64 twin: computed once, read by every test of the case"""
    c = _case(name)
    return c.twin(c.state)


def _counts(c, bx):
    return npth.cq_engine_counts(("critic", "policy"), bx, _nc(), c.O, c.ph, c.Oc + c.A, c.qh, c.E, c.B)


def _gemm_rows(ctx):
    return [q for q in ctx.prof_rows() if q["kernel"] in GEMMS]


@pytest.mark.parametrize("name", cc.NAMES)
def test_pair_of_updates_matches_the_twin(ctx, dev, name):
    c = _case(name)
    _, new, met, infos = _reference(name)
    assert all(i["vmin"] >= m.VAR_FLOOR and not i["warmed"] for i in infos), name
    r = m.Run(ctx, dev, c, c.state)
    assert (r.q_count, r.pi_count) == (1, 1)
    m.check(c, r, new, met, name)                                              # the one-step bars: no float32 gap enters
    assert r.metrics[9] == 0.0 and np.all(np.isfinite(r.metrics)) and all(np.all(np.isfinite(v)) for v in r.out.values())
    if name == "ties":
        n, s = c.qs.n_params, c.qs.n_stats
        for k, w in (("qp", n), ("qm", n), ("qv", n), ("qs", s)):
            assert np.array_equal(r.out[k][2 * w:3 * w], r.out[k][:w]) and not np.array_equal(r.out[k][w:2 * w], r.out[k][:w]), k


@pytest.mark.parametrize("name", ["half_split", "e16_cut"])
def test_engines(ctx, dev, name):
    """every profiled trunk GEMM row against the mirror's launches per engine.  half_split: the joint pass alone is on the
    split-operand engine; e16_cut: the shape of the layer at which each update's image list ends shows on both engines"""
    c = _case(name)
    bx = ctx.get_counter("gemm_bx") == 1
    m.Run(ctx, dev, c, c.state, prof=True)
    rows = _gemm_rows(ctx)
    print(f"crossq {name} gemm rows:", sorted((q["kernel"], q["engine"], q["M"], q["N"], q["K"], q["launches"]) for q in rows))
    npth.check_engine_counts(rows, _counts(c, bx))
    if not bx:
        assert all(q["engine"] == 0 for q in rows), rows
        return
    seen = lambda key: {q["engine"] for q in rows if (q["kernel"], q["M"], q["N"], q["K"]) == key}
    if name == "half_split":
        assert {q["engine"] for q in rows if c.B in (q["M"], q["K"])} == {0} and seen(("k_gemm_fwd", 2 * c.B, 128, 256)) == {1}
    else:
        assert seen(("k_gemm_fwd", 2 * c.B, 192, 128)) == {0, 1} and seen(("k_gemm_fwd", c.B, 128, 64)) == {0, 1}


@pytest.mark.parametrize("name", ["act64", "half_split", "many_rows"])
def test_two_identical_calls_give_identical_bits(ctx, dev, name):
    c = _case(name)
    assert m.Run(ctx, dev, c, c.state).same_bits(m.Run(ctx, dev, c, c.state)), name


def test_split_engine_off_meets_the_same_bars(ctx, dev):
    """gemm_bx 0: the joint pass of 4098 rows on the exact engine too, same bars"""
    c = _case("half_split")
    _, new, met, _ = _reference("half_split")
    was = ctx.get_counter("gemm_bx")
    ctx.set_option("gemm_bx", 0)
    try:
        assert ctx.get_counter("gemm_bx") == 0
        r = m.Run(ctx, dev, c, c.state, prof=True)
        rows = _gemm_rows(ctx)
    finally:
        ctx.set_option("gemm_bx", was)
    m.check(c, r, new, met, "half_split, split-operand engine off")
    assert rows and all(q["engine"] == 0 for q in rows), rows
    npth.check_engine_counts(rows, _counts(c, False))


@pytest.mark.parametrize("name,N", [("wide_policy", 5), ("act64", 37)])
def test_acting(ctx, dev, name, N):
    """rlx_crossq_act_f32, deterministic and sampled, on the case's policy with the parameters and statistics its pair of updates
    leaves, at test_gpu_crossq.py test_acting's 2e-6: a policy (2048, 1984) wide, and the A 64 head over three layers"""
    c = _case(name)
    new = _reference(name)[1]
    pp, pst = np.asarray(new["pp"], np.float32), np.asarray(new["ps"], np.float32)
    obs = np.random.default_rng([N, c.A]).standard_normal((N, c.O)).astype(np.float32)
    k1, eps = tw.key_chain(m.KEY, (N, c.A))
    tp, ts, to = m._t(pp, dev), m._t(pst, dev), m._t(obs, dev)
    for det in (True, False):
        out = torch.full((N, c.A), 7.0, device=dev)
        key = ctx.crossq_act(c.pd, tp, ts, to, m.KEY, out, c.hp(), deterministic=det)
        assert np.array_equal(key, k1)
        exp = tw.act(c.ps, pp.astype(np.float64), pst.astype(np.float64), obs.astype(np.float64), eps, c.h, det)
        got = out.cpu().numpy()
        print(f"crossq acting {name} N={N} deterministic={det}: {np.abs(got - exp).max():.2e}")
        assert np.abs(got - exp).max() <= 2e-6, (name, det, np.abs(got - exp).max())
    assert np.array_equal(ts.cpu().numpy(), pst) and np.array_equal(tp.cpu().numpy(), pp)


# ----------------------------------------------------------------------------------------------------------------------- refusals
REFUSALS = [("a_65", -4, "act_dim"), ("p_layers0", -1, "1..3 hidden layers"), ("q_layers0", -1, "1..3 hidden layers"),
            ("p_layers4", -1, "1..3 hidden layers"), ("q_layers4", -1, "1..3 hidden layers"), ("q_out_2", -1, "qdesc->out_dim must be 1"),
            ("q_in_a", -1, "qdesc->in_dim must be critic obs + act_dim"), ("warmup_neg", -1, "brn_warmup_steps")]


def _base_call_succeeds(ctx, dev):
    c = m.Case("base")
    r = m.Run(ctx, dev, c, c.state)
    assert r.metrics[9] == 0.0 and np.all(np.isfinite(r.metrics)) and np.any(r.out["qp"] != np.asarray(c.state["qp"], np.float32))


@pytest.mark.parametrize("what,code,word", REFUSALS)
def test_refusals_write_nothing(ctx, dev, what, code, word):
    """outside the envelope, where test_gpu_crossq.py has no case: the documented code and message from both updates, nothing written,
    and the context serves a valid call afterwards"""
    c = m.Case("base")
    hp = c.hp()
    relu = lambda i, h, o: L.mlp_desc(i, h, o, nets.ACT_RELU, False, False)
    hidden = [] if what.endswith("layers0") else [64, 64, 64, 64]
    if what == "a_65":
        c.pd, c.qd = relu(c.O, [64, 64], 130), relu(c.Oc + 65, [64, 64], 1)
    elif what.startswith("p_layers"):
        c.pd = relu(c.O, hidden, 2 * c.A)
    elif what.startswith("q_layers"):
        c.qd = relu(c.Oc + c.A, hidden, 1)
    elif what == "q_out_2":
        c.qd = relu(c.Oc + c.A, [64, 64], 2)
    elif what == "q_in_a":
        c.qd = relu(c.A, [64, 64], 1)
    elif what == "warmup_neg":
        hp = c.hp(brn_warmup_steps=-1)
    t = {k: m._t(c.state[k], dev) for k in tw.STATE_KEYS}
    before = {k: v.clone() for k, v in t.items()}
    met = torch.full((10,), 7.0, device=dev)
    batch = tuple(m._t(x, dev) for x in c.batch)
    calls = (lambda: ctx.crossq_critic_update(c.pd, t["pp"], t["ps"], c.qd, t["qp"], t["qm"], t["qv"], t["qs"], t["la"], batch, m.KEY, 0, hp, met),
             lambda: ctx.crossq_policy_update(c.pd, t["pp"], t["pm"], t["pv"], t["ps"], c.qd, t["qp"], t["qs"], t["la"], t["am"], t["av"],
                                              batch[0], m.KEY, 0, hp, met))
    for call in calls:
        with pytest.raises(RlxError) as err:
            call()
        assert f"rc={code}" in str(err.value) and word in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], before[k]) for k in t) and bool((met == 7.0).all())
    _base_call_succeeds(ctx, dev)


@pytest.mark.parametrize("what,code,word", [("n_0", -1, "N must be positive"), ("a_65", -1, "act_dim at most 64"), ("layers4", -1, "1..3 hidden layers")])
def test_acting_refusals_write_nothing(ctx, dev, what, code, word):
    c = m.Case("base")
    N = 0 if what == "n_0" else 4
    pd = {"a_65": L.mlp_desc(c.O, [64, 64], 130, nets.ACT_RELU, False, False),
          "layers4": L.mlp_desc(c.O, [64, 64, 64, 64], 2 * c.A, nets.ACT_RELU, False, False)}.get(what, c.pd)
    x = torch.full((4096,), 7.0, device=dev)                                   # every pointer: nothing of it may change
    key, f = L._key_arr(m.KEY), torch.float32
    with pytest.raises(RlxError) as err:
        L._check(ctx.lib.rlx_crossq_act_f32(ctx.h, ctypes.byref(pd), L._ptr(x, f), L._ptr(x, f), L._ptr(x, f), ctypes.c_int64(N), key, 1, L._ptr(x, f), 0,
                                            ctypes.byref(c.hp()), L._stream()), "rlx_crossq_act_f32")
    assert f"rc={code}" in str(err.value) and word in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and (key[0], key[1]) == tuple(int(v) for v in m.KEY)
    _base_call_succeeds(ctx, dev)
