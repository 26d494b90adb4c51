"""GPU: MPO (mpo.hip) against the reference fixture (tests/golden/mpo_reference.npz) and the float64 twin (tests/mpo_twin.py): acting
and one whole update per fixture case, the twin at the reference defaults (obs 48, act 12, B 256 and 4096, S 20, hidden 256, 51
atoms), bit-identical repeats, the refusals just outside the envelope, an ill-conditioned temperature, and the plugin end to end.
A fixture case with a second `update` call is also checked at step 2, started from the twin's state after the first call.
Tolerances (tests/mpo_cases.py): 1e-5 relative (L2 per vector); second Adam moments 5e-5 (float32's 1 - b2); the expected-q
metric with a floor of max|v| / 10 (its value is a difference of atoms that large)."""
import numpy as np
import pytest
import torch

import mpo_cases
import mpo_twin as tw
from mpo_cases import Run, _check_metrics, _hp, _rel, _t
from rlx_amd.hip import mpo_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", range(mpo_cases.n_cases()))
def test_act_matches_the_reference(ctx, dev, c):
    fc = mpo_cases.load(c)
    z, k = fc.z, fc.k
    desc = mpo_desc(fc.Op, fc.Oc, fc.A, fc.H, fc.NA)
    hp = _hp(fc.h)
    obs = fc.batch[0]
    N = obs.shape[0]
    P = _t(fc.state["p"], dev)
    pidx = _t(fc.pidx, dev, np.int32) if fc.full_obs else None
    act, proc = torch.empty(N, fc.A, device=dev), torch.empty(N, fc.A, device=dev)
    low, high = _t(fc.low, dev), _t(fc.high, dev)
    key = L.prng_key(3)
    eps, x = _t(fc.eps_act, dev), _t(obs, dev)       # both alive across the call (the library holds the noise pointer)
    ctx.dbg_set_sac_noise(eps, None)
    try:
        ctx.mpo_act(desc, P, x, key, act, proc, hp, low, high, pidx=pidx)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    assert _rel(act.cpu().numpy(), z[k + "act_sample"]) < 1e-5 and _rel(proc.cpu().numpy(), z[k + "act_sample_proc"]) < 1e-5
    k2 = ctx.mpo_act(desc, P, _t(obs, dev), key, act, proc, hp, low, high, deterministic=True, pidx=pidx)
    assert np.array_equal(k2, key)
    assert _rel(proc.cpu().numpy(), z[k + "act_det_proc"]) < 1e-5 and _rel(act.cpu().numpy(), z[k + "act_mean"]) < 1e-5
    k3 = ctx.mpo_act(desc, P, _t(obs, dev), key, act, proc, hp, low, high, pidx=pidx)
    assert not np.array_equal(k3, key) and torch.isfinite(act).all()


@pytest.mark.parametrize("c", range(mpo_cases.n_cases()))
def test_update_matches_the_reference(ctx, dev, c):
    fc = mpo_cases.load(c)
    z, k = fc.z, fc.k
    desc = mpo_desc(fc.Op, fc.Oc, fc.A, fc.H, fc.NA)
    pidx, cidx = (fc.pidx, fc.cidx) if fc.full_obs else (None, None)
    r = Run(ctx, dev, desc, fc.state, fc.batch, fc.h, (fc.eps_c, fc.eps_a), pidx, cidx)
    _check_metrics(r.metrics, z[k + "metrics"], max(abs(fc.h["v_min"]), abs(fc.h["v_max"])))
    for name, key, tol in (("p_after", "p", 1e-5), ("pm_after", "pm", 1e-5), ("pv_after", "pv", 5e-5), ("q_after", "q", 1e-5),
                           ("qm_after", "qm", 1e-5), ("qv_after", "qv", 5e-5)):
        idx, val, _ = fc.sampled(name)
        assert _rel(r.out[key][idx], val) < tol, (name, _rel(r.out[key][idx], val))
    assert _rel(r.out["d"], z[k + "duals_after"]) < 1e-5
    assert _rel(r.out["dm"], z[k + "duals_exp_avg"]) < 1e-5 and _rel(r.out["dv"], z[k + "duals_exp_avg_sq"]) < 5e-5
    A = fc.A
    assert r.out["d"][1:1 + A].tobytes() == fc.state["d"][1:1 + A].astype(np.float32).astype(np.float64).tobytes()   # no gradient
    assert np.array_equal(r.out["tp"], fc.state["tp"]) and np.array_equal(r.out["tq"], fc.state["tq"])             # read only


@pytest.mark.parametrize("c", mpo_cases.two_call_cases())
def test_second_update_matches_the_reference(ctx, dev, c):
    """the fixture's second `update` (step 2, the reference's Adam moments and duals carried over), teacher-forced: the library
    starts from the twin's state after the first call, so the bars measure the kernels, not two steps of drift"""
    fc = mpo_cases.load(c)
    sc = fc.second
    desc = mpo_desc(fc.Op, fc.Oc, fc.A, fc.H, fc.NA)
    pidx, cidx = fc.indices()
    st1, _, _ = tw.update(fc.state, fc.LP, fc.LQ, fc.batch, fc.eps_c, fc.eps_a, fc.h, 1, pidx, cidx)
    assert np.any(st1["pm"] != 0) and np.any(st1["qv"] != 0) and np.any(st1["dm"] != 0)
    r = Run(ctx, dev, desc, st1, fc.batch, fc.h, (sc.eps_c, sc.eps_a), pidx, cidx, step=2)
    _check_metrics(r.metrics, sc.metrics, max(abs(fc.h["v_min"]), abs(fc.h["v_max"])))
    for name, key, tol in (("p_after", "p", 1e-5), ("pm_after", "pm", 1e-5), ("pv_after", "pv", 5e-5), ("q_after", "q", 1e-5),
                           ("qm_after", "qm", 1e-5), ("qv_after", "qv", 5e-5)):
        idx, val, _ = sc.sampled(name)
        assert _rel(r.out[key][idx], val) < tol, (name, _rel(r.out[key][idx], val))
    assert _rel(r.out["d"], sc.duals) < 1e-5
    assert _rel(r.out["dm"], sc.dm) < 1e-5 and _rel(r.out["dv"], sc.dv) < 5e-5
    mpo_cases.check_dual_step(r.out["d"], sc.duals, st1["d"])        # step 2's bias corrections


def _defaults_case(B, seed, A=12, O=48):
    h = dict(tw.HP)
    S, H, NA = h["action_sampling_number"], 256, 51
    rng = np.random.default_rng(seed)
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    p, q = tw.make_params(seed, O, O, A, H, NA)
    tp, tq = tw.make_params(seed + 1, O, O, A, H, NA)
    zp, zq, nd = np.zeros(p.size), np.zeros(q.size), 2 * A + 2
    st = dict(p=p, pm=zp, pv=zp, tp=tp, q=q, qm=zq, qv=zq, tq=tq, d=tw.init_duals(A, h), dm=np.zeros(nd), dv=np.zeros(nd))
    dones = (rng.random(B) < 0.2).astype(np.float64)
    truncs = dones * (rng.random(B) < 0.5)
    batch = (f32(rng.standard_normal((B, O))), f32(rng.standard_normal((B, O))), f32(rng.standard_normal((B, A)) * 0.8),
             f32(rng.standard_normal(B) * 5.0), dones, truncs, rng.integers(1, 5, B).astype(np.float64))
    eps = (f32(rng.standard_normal((S, B, A))), f32(rng.standard_normal((S, 2 * B, A))))
    return h, st, batch, eps, mpo_desc(O, O, A, H, NA)


@pytest.mark.parametrize("B", [256, 4096])
def test_update_matches_the_twin_at_the_reference_defaults(ctx, dev, B):
    h, st, batch, eps, desc = _defaults_case(B, 11 + B)
    LP, LQ = tw.policy_layout(48, 12, 256), tw.critic_layout(48, 12, 256, 51)
    r = Run(ctx, dev, desc, st, batch, h, eps)
    new, met, _ = tw.update(st, LP, LQ, batch, eps[0], eps[1], h, 1)
    _check_metrics(r.metrics, met, 1600.0)
    for key, tol in (("p", 1e-5), ("pm", 1e-5), ("pv", 5e-5), ("q", 1e-5), ("qm", 1e-5), ("qv", 5e-5), ("d", 1e-5), ("dm", 1e-5),
                     ("dv", 5e-5)):
        assert _rel(r.out[key], new[key]) < tol, (key, _rel(r.out[key], new[key]))


def test_two_identical_calls_give_identical_bits(ctx, dev):
    h, st, batch, _, desc = _defaults_case(512, 5)
    a, b = Run(ctx, dev, desc, st, batch, h, key=(1, 2)), Run(ctx, dev, desc, st, batch, h, key=(1, 2))
    assert np.array_equal(a.key, b.key) and a.metrics.tobytes() == b.metrics.tobytes()
    for k in a.out:
        assert a.out[k].tobytes() == b.out[k].tobytes(), k
    assert np.all(np.isfinite(a.metrics))


def test_ill_conditioned_temperature_stays_finite(ctx, dev):
    """log_eta at its minimum (eta ~ 2.5e-8): float32 rounding of q legitimately changes the softmax (it is one-hot at the argmax),
    so nothing is compared to the twin; the update stays finite and loss_eta is finite"""
    h, st, batch, eps, desc = _defaults_case(256, 9)
    st = dict(st, d=st["d"].copy())
    st["d"][0] = -18.0
    r = Run(ctx, dev, desc, st, batch, h, eps)
    assert np.all(np.isfinite(r.metrics)) and np.isfinite(r.metrics[3])
    for k in ("p", "q", "d", "pm", "pv"):
        assert np.all(np.isfinite(r.out[k])), k
    _, met, ex = tw.update(st, tw.policy_layout(48, 12, 256), tw.critic_layout(48, 12, 256, 51), batch, eps[0], eps[1], h, 1)
    wq = ex["weights_q"]
    assert np.all(np.isfinite(wq)) and np.allclose(wq.max(0), 1.0)            # one-hot in the twin too


@pytest.mark.parametrize("field, value", [("hidden", 576), ("hidden", 96), ("nr_atoms", 129), ("nr_atoms", 1), ("act_dim", 65),
                                          ("S", 65), ("S", 0)])
def test_refusals_just_outside_the_envelope(ctx, dev, field, value):
    h, st, batch, eps, _ = _defaults_case(8, 3, A=4, O=8)
    dims = dict(hidden=256, nr_atoms=51, act_dim=4)
    if field in dims:
        dims[field] = value
    if field == "S":
        h = dict(h, action_sampling_number=value)
    desc = mpo_desc(8, 8, dims["act_dim"], dims["hidden"], dims["nr_atoms"])
    with pytest.raises(L.RlxError):
        Run(ctx, dev, desc, st, batch, h)
    obs = _t(batch[0], dev)
    a = torch.empty(8, max(dims["act_dim"], 1), device=dev)
    with pytest.raises(L.RlxError):
        ctx.mpo_act(desc, torch.zeros(100000, device=dev), obs, L.prng_key(0), a, a.clone(), _hp(h), _t(np.full(4, -1.0), dev),
                    _t(np.ones(4), dev))


def _mpo_plugin(env_name, env_over, alg_over, pidx=None, cidx=None):
    from rlx_amd.runner.config_dict import ConfigDict
    from rlx_amd.runner.default_config import get_config as runner_cfg
    import rlx_amd.algorithms.mpo.hip  # noqa: F401
    import rlx_amd.environments.synthetic.random_obs, rlx_amd.environments.synthetic.numpy_obs  # noqa: F401,E401
    from rlx_amd.algorithms.algorithm_manager import get_algorithm_config, get_algorithm_model_class
    from rlx_amd.environments.environment_manager import get_environment_config, get_environment_create_train_and_eval_env
    config = ConfigDict()
    config.runner = runner_cfg("train")
    config.algorithm = get_algorithm_config("mpo.hip")
    config.environment = get_environment_config(env_name)
    for k, v in env_over.items():
        config.environment[k] = v
    for k, v in alg_over.items():
        config.algorithm[k] = v
    env, eval_env = get_environment_create_train_and_eval_env(env_name)(config)
    if pidx is not None:
        env.policy_observation_indices, env.critic_observation_indices = pidx, cidx
    return get_algorithm_model_class("mpo.hip"), config, env, eval_env


@pytest.mark.parametrize("env_name,indices", [("synthetic.random_obs", False), ("synthetic.numpy_obs", False),
                                              ("synthetic.random_obs", True)])
def test_plugin_trains_end_to_end(dev, tmp_path, env_name, indices):
    """`mpo.hip` end to end with small periods: warm-up actions, acting, the n-step ring, normaliser, updates, target copies, the env
    actor, the 17 metrics, evaluation and a save / load round trip"""
    import os
    pidx, cidx = (np.arange(0, 10), np.arange(4, 20)) if indices else (None, None)
    cls, config, env, eval_env = _mpo_plugin(env_name, dict(nr_envs=16, obs_dim=20, act_dim=3, horizon=10),
                                   dict(batch_size=32, buffer_size=16 * 8, learning_starts=16 * 3, n_steps=2, optimize_every_n_steps=2,
                                        target_network_update_period=7, actor_update_period=4, action_sampling_number=5,
                                        nr_hidden_units=64, total_timesteps=16 * 16, logging_frequency=16 * 8,
                                        evaluation_frequency=16 * 8), pidx, cidx)
    config.runner.save_model = True
    m = cls(config, env, eval_env, str(tmp_path), None)
    assert (m.desc.policy_obs_dim, m.desc.critic_obs_dim) == ((10, 16) if indices else (20, 20))
    p0, q0 = m.pparams.clone(), m.qparams.clone()
    m.train()
    met = m.last_metrics
    for name in tw.METRICS:
        assert name in met and np.isfinite(met[name]), (name, met)
    assert m.nr_updates == 7                                   # iterations 4, 6, ..., 16 optimise (global step > learning_starts)
    assert (m.pparams - p0).abs().max().item() > 0 and (m.qparams - q0).abs().max().item() > 0
    # the last update (7) is a target period: targets equal the online nets right after the copy; the env actor took the target
    # actor at iteration 16, before that copy -- the initial one
    assert torch.equal(m.tpparams, m.pparams) and torch.equal(m.tqparams, m.qparams)
    assert torch.equal(m.env_pparams, p0)
    assert "eval/episode_return" in met
    m.save()
    config.runner.load_model = os.path.join(str(tmp_path), "models", "best.model")
    m2 = cls.load(config, env, eval_env, str(tmp_path), None, [])
    for k in cls._STATE:
        assert torch.equal(getattr(m2, k), getattr(m, k)), k
    assert m2.nr_updates == m.nr_updates and len(m2.test(2)) <= 2
