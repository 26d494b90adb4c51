"""GPU: FastMPO (fastmpo.hip) through the C ABI against the float64 twin (tests/fastmpo_twin.py) with injected noise: acting in the
three rescaling modes, one whole update (P 2 x G 2) for every network kind, one and two critics, the clipped choice and action
clipping on and off, a second call continued from the twin's state, bit-identical repeats, and every refusal.
Tolerances: tests/fastmpo_cases.py (the project's own)."""
import numpy as np
import pytest
import torch

import fastmpo_cases as fc
import fastmpo_twin as tw
from fastmpo_cases import Case, Run, _rel, _t, f32
from rlx_amd.hip import fastmpo_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rescaling", ["none", "normal", "fastsac"])
@pytest.mark.parametrize("clip", [False, True])
def test_act_matches_the_twin(ctx, dev, rescaling, clip):
    c = Case(21, "fastsac", action_rescaling=rescaling, action_clipping=clip)
    rng = np.random.default_rng(5)
    N = 37
    obs, eps = f32(rng.standard_normal((N, c.O))), f32(rng.standard_normal((N, c.A)) * 2.0)
    low, high = f32(-1.0 - rng.random(c.A)), f32(0.5 + rng.random(c.A))
    scale = f32(0.5 + rng.random(c.A))
    hp = fc.hparams(c.h)
    lo, hi = {"none": (None, None), "normal": (_t(low, dev), _t(high, dev)), "fastsac": (_t(scale, dev), None)}[rescaling]
    P, x, e = _t(c.st["p"], dev), _t(obs, dev), _t(eps, dev)
    act, proc = torch.empty(N, c.A, device=dev), torch.empty(N, c.A, device=dev)
    key = L.prng_key(3)
    ctx.dbg_set_sac_noise(e, None)
    try:
        ctx.fastmpo_act(c.desc, P, x, key, act, proc, hp, lo, hi)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    a, pa = tw.act(c.st["p"], c.LP, obs, eps, c.h, low, high, scale)
    assert _rel(act.cpu().numpy(), a) < 1e-5 and _rel(proc.cpu().numpy(), pa) < 1e-5
    if clip:
        assert np.any(np.abs(a) > 1.0)                           # the clip acts
    k2 = ctx.fastmpo_act(c.desc, P, x, key, act, proc, hp, lo, hi, deterministic=True)
    a, pa = tw.act(c.st["p"], c.LP, obs, None, c.h, low, high, scale, deterministic=True)
    assert np.array_equal(k2, key)
    assert _rel(act.cpu().numpy(), a) < 1e-5 and _rel(proc.cpu().numpy(), pa) < 1e-5
    k3 = ctx.fastmpo_act(c.desc, P, x, key, act, proc, hp, lo, hi)      # the library's own draws
    assert not np.array_equal(k3, key) and torch.isfinite(act).all() and (act.cpu().numpy() != a).any()


@pytest.mark.parametrize("aclip", [False, True])
@pytest.mark.parametrize("E, clipped", [(1, False), (2, False), (2, True)])
@pytest.mark.parametrize("kind", ["fastsac", "fasttd3", "mpo"])
def test_whole_update_matches_the_twin(ctx, dev, kind, E, clipped, aclip):
    """obs 10, act 5, widths (128, 64, 64), 51 atoms, B 13, K 4, P 2 x G 2"""
    c = Case(100 + 7 * E + aclip, kind, E=E, clipped_double_q_learning=clipped, action_clipping=aclip)
    new, met, counts, ex = c.twin()
    if clipped:                                                  # both branches of the choice are taken
        v = ex["critic"]["value"]
        assert bool((v[0] <= v[1]).any()) and bool((v[0] > v[1]).any())
    r = Run(ctx, dev, c)
    fc.check_against_twin(r, new, met, counts, c.h, c.st, min_sel=fc.min_selected(c))
    assert counts == (4, 2, 2)
    assert np.any(r.out["d"][1:1 + c.A] != f32(c.st["d"][1:1 + c.A]))        # log_alpha_mean has a gradient and a step


def test_policy_and_critic_of_different_kinds(ctx, dev):
    c = Case(31, "fasttd3", policy_kind="mpo", E=2, action_clipping=True, policy_hidden=(64, 128, 64), critic_hidden=(192, 64, 128))
    new, met, counts, _ = c.twin()
    fc.check_against_twin(Run(ctx, dev, c), new, met, counts, c.h, c.st, min_sel=fc.min_selected(c))


@pytest.mark.parametrize("kind", ["fastsac", "mpo"])
def test_second_call_continues_from_the_twins_state(ctx, dev, kind):
    """teacher-forced: the library starts from the twin's state after a first call (non-zero moments in all three optimisers, moved
    targets and duals, optimiser counts (4, 2, 2)), with weight decay on the duals too"""
    c = Case(57, kind, E=2, clipped_double_q_learning=True, action_clipping=True, dual_weight_decay=0.01)
    st1, _, counts1, _ = c.twin()
    assert all(np.any(st1[k] != 0) for k in ("pm", "pv", "qm", "qv", "dm", "dv")) and counts1 == (4, 2, 2)
    st1 = {k: f32(v) for k, v in st1.items()}
    new, met, counts, _ = c.twin(st1, counts1)
    r = Run(ctx, dev, c, st1, counts1)
    fc.check_against_twin(r, new, met, counts, c.h, st1, min_sel=fc.min_selected(c))
    assert counts == (8, 4, 4)


@pytest.mark.parametrize("inject", [True, False])
def test_two_identical_calls_give_identical_bits(ctx, dev, inject):
    c = Case(77, "fastsac", E=2, B=300, clipped_double_q_learning=True, action_clipping=True)
    a, b = Run(ctx, dev, c, inject=inject), Run(ctx, dev, c, inject=inject)
    assert a.counts == b.counts and a.metrics.tobytes() == b.metrics.tobytes()
    for k in a.out:
        assert a.out[k].tobytes() == b.out[k].tobytes(), k
    assert np.all(np.isfinite(a.metrics))
    if not inject:                                              # another noise key: other draws
        d = Run(ctx, dev, c, inject=False, key=(3, 8))
        assert d.out["q"].tobytes() != a.out["q"].tobytes()


REFUSALS = [("hp", dict(clipped_double_q_learning=True), dict(E=1)), ("hp", dict(action_sampling_number=0), {}),
            ("hp", dict(action_sampling_number=65), {}), ("desc", dict(act_dim=65), {}), ("desc", dict(act_dim=0), {}),
            ("desc", dict(nr_atoms=1), {}), ("desc", dict(nr_atoms=129), {}), ("desc", dict(critic_hidden=(96, 64, 64)), {}),
            ("desc", dict(policy_hidden=(64, 64, 1088)), {}), ("desc", dict(critic_hidden=(832, 64, 64)), {}),       # behind LayerNorm + SiLU
            ("desc", dict(critic_kind=2, critic_hidden=(576, 64, 64)), {}), ("desc", dict(policy_kind=3), {}),
            ("desc", dict(critic_kind=-1), {}), ("hp", dict(nr_policy_updates_per_step=0), {}),
            ("hp", dict(nr_critic_updates_per_policy_update=0), {}), ("hp", dict(v_max=-20.0), {})]


@pytest.mark.parametrize("where, change, case", REFUSALS)
def test_refusals_outside_the_envelope(ctx, dev, where, change, case):
    c = Case(3, "fastsac", B=8, **case)
    h, desc = dict(c.h), c.desc
    if where == "hp":
        h.update(change)
    else:
        args = dict(act_dim=c.A, nr_atoms=c.NA, policy_kind=0, critic_kind=0, policy_hidden=(128, 64, 64), critic_hidden=(128, 64, 64))
        args.update(change)
        desc = fastmpo_desc(c.O, c.O, args["act_dim"], args["nr_atoms"], c.E == 2, args["policy_kind"], args["critic_kind"],
                            args["policy_hidden"], args["critic_hidden"])
    before = {k: v.copy() for k, v in c.st.items()}
    with pytest.raises(L.RlxError):
        Run(ctx, dev, c, h=h, desc=desc)
    if where == "desc" or "action_sampling_number" in change or "clipped_double_q_learning" in change:
        obs = _t(c.batches[0][0], dev)
        a = torch.empty(c.B, 64, device=dev)
        with pytest.raises(L.RlxError):
            ctx.fastmpo_act(desc, torch.zeros(1 << 20, device=dev), obs, L.prng_key(0), a, a.clone(), fc.hparams(h))
    for k, v in before.items():
        assert np.array_equal(c.st[k], v)


def test_update_refuses_rescaling_and_index_mistakes(ctx, dev):
    c = Case(3, "fastsac", B=8)
    obs = _t(c.batches[0][0], dev)
    a = torch.empty(c.B, c.A, device=dev)
    P = _t(c.st["p"], dev)
    for mode in ("normal", "fastsac"):                           # the rescaling operands are missing
        with pytest.raises(L.RlxError):
            ctx.fastmpo_act(c.desc, P, obs, L.prng_key(0), a, a.clone(), fc.hparams(dict(c.h, action_rescaling=mode)))
    narrow = fastmpo_desc(c.O - 2, c.O, c.A, c.NA, True, 0, 0, (128, 64, 64), (128, 64, 64))
    with pytest.raises(L.RlxError):                               # policy_obs_dim != O without column indices
        ctx.fastmpo_act(narrow, P, obs, L.prng_key(0), a, a.clone(), fc.hparams(c.h))
    with pytest.raises(L.RlxError):
        Run(ctx, dev, c, desc=narrow)
