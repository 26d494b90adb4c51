"""GPU: rlx_dtrl_update_f32 against the twin's loss + oracle/ppo.py's float64 clip + Adam over the update cases of tests/dtrl_cases.py
-- one step; three minibatches from opt_count 3 with non-zero moments; A = 16 with hp->critic_states and computed rollout means; both
networks clipped at every step; the other permutation scheme; a prefetched permutation; a step the device skips -- with
test_gpu_dtrl_update.py's comparisons and bars (tests/espo_cases.py's: metrics 1e-5 of max(|value|, 1); vectors 1e-5 relative L2, second
moments 5e-5, the parameter step 2e-4), and the refusals of the update's own checks."""
import numpy as np
import pytest
import torch

import dtrl_cases as dc
from rlx_amd.hip import lib as L
from test_gpu_dtrl import hparams
from test_gpu_dtrl_shapes import REFUSAL_BASE, descs, refused_call

pytestmark = pytest.mark.gpu
n64 = lambda x: x.cpu().numpy().astype(np.float64)


def run_update(ctx, dev, u, prefetch=False):
    """one call from the case's start state -> (metrics [n_upd, 14], [p, pm, pv, q, cm, cv] device tensors, new key, new count)"""
    b = u.built
    c, B = b["c"], u.B
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    sh = lambda x: t(x).view(1, B, -1) if np.ndim(x) == 2 else t(x).view(1, B)
    state = [t(v) for v in b["start"]]
    p, pm, pv, q, cm, cv = state
    out = torch.full((u.n_upd, 14), 7.0, device=dev)
    cst = None if c["cstates"] is None else t(c["cstates"])
    pd, cd = descs(c)
    if prefetch:
        ctx.ppo_prefetch_permutation(b["key"].copy(), u.E, B, u.scheme)
    key, count = ctx.dtrl_update(pd, p, pm, pv, cd, q, cm, cv, sh(c["states"]), sh(c["actions"]), sh(c["old_means"]) if u.given else None,
                                 sh(c["logp_old"]), sh(c["returns"]), sh(c["adv"]), u.E, u.mb, b["key"].copy(), u.opt_count0, b["lrs"],
                                 c["global_step"], hparams(c["h"], None if cst is None else cst.data_ptr()), out, scheme=u.scheme)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), state, key, count


def check_net(name, what, st, par, m1, m2, p0):
    sel = np.abs(st.m) > 1e-3 * np.sqrt(np.mean(st.m ** 2))
    fig = (dc.rel(n64(par), st.params), dc.rel(n64(m1), st.m), dc.rel(n64(m2), st.v), dc.rel((n64(par) - p0)[sel], (st.params - p0)[sel]))
    print("dtrl update shape figures:", name, what, ["%.2e" % v for v in fig])
    assert fig[0] < 1e-5 and fig[1] < 1e-5 and fig[2] < 5e-5 and fig[3] < 2e-4, (name, what, fig)


@pytest.mark.parametrize("name", ["e1_m1", "e2_m3_count3", "a16_cstates_null_means", "both_clipped", "other_scheme"])
def test_update_matches_the_twin_over_the_cases(ctx, dev, name):
    u = dc.UPDATES[name]
    b = u.built
    met, infos, ps, cs = b["twin"]
    perm = torch.zeros(u.E, u.B, dtype=torch.int32, device=dev)
    key_e = ctx.permutation(b["key"].copy(), perm.view(-1), u.E, u.B, u.scheme)
    assert np.array_equal(perm.cpu().numpy().reshape(u.n_upd, u.mb), b["idx"])         # the rows the twin stepped on
    got, (p, pm, pv, q, cm, cv), key, count = run_update(ctx, dev, u)
    assert count == u.opt_count0 + u.n_upd and np.array_equal(key, b["key_out"]) and np.array_equal(key, key_e)
    print("dtrl update shapes, |got - twin| / max(|twin|, 1) per step:", name, "\n", np.abs(got - met) / np.maximum(np.abs(met), 1.0))
    assert np.all(np.abs(got - met) <= 1e-5 * np.maximum(np.abs(met), 1.0)), np.abs(got - met).max(0)
    check_net(name, "policy", ps, p, pm, pv, b["start"][0].astype(np.float64))
    check_net(name, "critic", cs, q, cm, cv, b["start"][3].astype(np.float64))


def test_a_prefetched_permutation_changes_no_bit(ctx, dev):
    """the pf_valid branch: the same call from the same state, once behind rlx_ppo_prefetch_permutation with the same key, E, B and
    scheme"""
    u = dc.UPDATES["prefetch"]
    plain, fetched = run_update(ctx, dev, u), run_update(ctx, dev, u, prefetch=True)
    assert plain[3] == fetched[3] == u.n_upd and np.array_equal(plain[2], fetched[2]) and np.array_equal(plain[2], u.built["key_out"])
    assert np.array_equal(plain[0].astype(np.float32).view(np.uint32), fetched[0].astype(np.float32).view(np.uint32))
    for a, b_ in zip(plain[1], fetched[1]):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
    met = u.built["twin"][0]
    assert np.all(np.abs(plain[0] - met) <= 1e-5 * np.maximum(np.abs(met), 1.0))


@pytest.mark.parametrize("name", ["skip_critic", "skip_policy"])
def test_a_non_finite_gradient_norm_skips_that_networks_step_alone(ctx, dev, name):
    """returns[0] = nan: the critic's parameters and moments keep their bits and the policy steps as the twin does; advantages[0] =
    inf: the mirror image.  (The twin's optimiser does not skip: the untouched side is compared with its inputs.)"""
    u = dc.UPDATES[name]
    b = u.built
    met, _, ps, cs = b["twin"]
    got, (p, pm, pv, q, cm, cv), _, count = run_update(ctx, dev, u)
    assert count == 1
    t = lambda v: torch.from_numpy(v).to(dev)
    skipped, start, stepped, st, i_norm = (((q, cm, cv), b["start"][3:], (p, pm, pv), ps, 12) if name == "skip_critic" else
                                           ((p, pm, pv), b["start"][:3], (q, cm, cv), cs, 13))
    for x, x0 in zip(skipped, start):
        assert torch.equal(x.view(torch.int32), t(x0).view(torch.int32))
    assert not np.isfinite(got[0, 25 - i_norm]) and abs(got[0, i_norm] - met[0, i_norm]) <= 1e-5 * max(met[0, i_norm], 1.0)
    check_net(name, "the stepped network", st, *stepped, b["start"][0 if name == "skip_critic" else 3].astype(np.float64))


@pytest.mark.parametrize("name", list(dc.REFUSED_UPDATE))
def test_update_refuses_what_its_checks_refuse(ctx, dev, name):
    change, code, field = dc.REFUSED_UPDATE[name]
    c = dc.CASES[REFUSAL_BASE].c
    pd, cd, hp, extra = refused_call(c, change)
    B = c["actions"].shape[0]
    mb = extra.get("mb", B)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    sh = lambda x: t(x).view(1, B, -1) if np.ndim(x) == 2 else t(x).view(1, B)
    n = 1 << 20
    state = [torch.full((n,), 7.0, device=dev) for _ in range(6)]
    out = torch.full((4, 14), 7.0, device=dev)
    key = L.prng_key(5)
    try:
        if "world" in extra:
            ctx.set_rank(0, extra["world"])
        with pytest.raises(L.RlxError) as e:
            ctx.dtrl_update(pd, state[0], state[1], state[2], cd, state[3], state[4], state[5], sh(c["states"]), sh(c["actions"]),
                            sh(c["old_means"]), sh(c["logp_old"]), sh(c["returns"]), sh(c["adv"]), extra.get("E", 1), mb, key,
                            extra.get("opt_count", 0), np.full(4, 1e-3, np.float32), c["global_step"], hp, out)
    finally:
        if "world" in extra:
            ctx.set_rank(0, 1)
    torch.cuda.synchronize()
    assert "rc=%d)" % code in str(e.value) and field in str(e.value) and "rlx_dtrl_update_f32" in str(e.value), str(e.value)
    assert all(bool((x == 7.0).all()) for x in state) and bool((out == 7.0).all()) and np.array_equal(key, L.prng_key(5))
