"""CPU: the float64 MPO twin (tests/mpo_twin.py) against the reference fixture (tests/golden/mpo_reference.npz, outputs of the
reference's own modules and `update` closure; one case runs two consecutive calls), the reference quirks the fixture pins, and the
plugin's registration."""
import os

import numpy as np
import pytest
import torch

import mpo_cases
import mpo_twin as tw

REF = os.environ.get("RLX_REFERENCE", "/root/reference")
HAVE_REF = os.path.isdir(os.path.join(REF, "rl_x/algorithms/mpo/pytorch"))


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


def test_layouts_and_library_param_counts():
    from rlx_amd.hip import MpoDesc, MpoHparams, mpo_desc
    from rlx_amd.hip import lib as L
    import ctypes
    LP, LQ = tw.policy_layout(48, 12, 256), tw.critic_layout(48, 12, 256, 51)
    assert LP["n"] == (48 * 256 + 3 * 256) + 2 * (256 * 256 + 256) + (256 * 24 + 24)
    assert LQ["n"] == (60 * 256 + 3 * 256) + 2 * (256 * 256 + 256) + (256 * 51 + 51)
    lib = L.load_library()
    d = mpo_desc(48, 48, 12, 256, 51)
    assert lib.rlx_mpo_param_count(ctypes.byref(d), 0) == LP["n"]
    assert lib.rlx_mpo_param_count(ctypes.byref(d), 1) == LQ["n"]
    assert lib.rlx_mpo_param_count(ctypes.byref(d), 2) == 2 * 12 + 2
    assert ctypes.sizeof(MpoDesc) == 20 and ctypes.sizeof(MpoHparams) == 16 * 4 + 3 * 4      # include/rlx_hip.h


def test_fixture_is_inputs_and_outputs_only():
    z = np.load(mpo_cases.FIXTURE)
    assert str(z["source"]).startswith("reference:rl_x/algorithms/mpo/pytorch")
    assert not os.path.basename(mpo_cases.FIXTURE).startswith("reference_")
    assert os.path.getsize(mpo_cases.FIXTURE) < 1 << 20


@pytest.mark.parametrize("c", range(mpo_cases.n_cases()))
def test_twin_reproduces_the_reference_fixture(c):
    fc = mpo_cases.load(c)
    z, k = fc.z, fc.k
    # acting (policy.py:71-97)
    mean, std = tw.policy_get_action(tw._t(fc.state["p"]), fc.LP, tw._t(fc.batch[0][:, fc.pidx]), fc.h)
    assert _rel(mean.detach().numpy(), z[k + "act_mean"]) < 1e-12 and _rel(std.detach().numpy(), z[k + "act_std"]) < 1e-12
    a, pa = tw.act(fc.state["p"], fc.LP, fc.batch[0][:, fc.pidx], fc.eps_act, fc.h, fc.low, fc.high)
    assert _rel(a, z[k + "act_sample"]) < 1e-12 and _rel(pa, z[k + "act_sample_proc"]) < 1e-12
    _, pd = tw.act(fc.state["p"], fc.LP, fc.batch[0][:, fc.pidx], None, fc.h, fc.low, fc.high, deterministic=True)
    assert _rel(pd, z[k + "act_det_proc"]) < 1e-12
    # one update
    pidx, cidx = fc.indices()
    new, met, _ = tw.update(fc.state, fc.LP, fc.LQ, fc.batch, fc.eps_c, fc.eps_a, fc.h, 1, pidx, cidx)
    ref = z[k + "metrics"]
    assert np.all(np.abs(met - ref) <= 1e-12 * np.maximum(np.abs(ref), 1.0)), (met, ref)
    for name, key in (("p_after", "p"), ("pm_after", "pm"), ("pv_after", "pv"), ("q_after", "q"), ("qm_after", "qm"), ("qv_after", "qv")):
        idx, val, norm = fc.sampled(name)
        assert _rel(new[key][idx], val) < 1e-12, name
        assert abs(np.linalg.norm(new[key]) - norm) <= 1e-12 * max(norm, 1e-30), name
    assert _rel(new["d"], z[k + "duals_after"]) < 1e-12
    assert _rel(new["dm"], z[k + "duals_exp_avg"]) < 1e-12 and _rel(new["dv"], z[k + "duals_exp_avg_sq"]) < 1e-12


@pytest.mark.parametrize("c", mpo_cases.two_call_cases())
def test_twin_reproduces_the_second_update(c):
    """the fixture's second `update` call (step 2; the reference's three Adam optimisers carry their moments over, the duals
    their values): the twin from its own state after the first call"""
    fc = mpo_cases.load(c)
    sc = fc.second
    pidx, cidx = fc.indices()
    st1, _, _ = tw.update(fc.state, fc.LP, fc.LQ, fc.batch, fc.eps_c, fc.eps_a, fc.h, 1, pidx, cidx)
    new, met, _ = tw.update(st1, fc.LP, fc.LQ, fc.batch, sc.eps_c, sc.eps_a, fc.h, 2, pidx, cidx)
    assert np.all(np.abs(met - sc.metrics) <= 1e-12 * np.maximum(np.abs(sc.metrics), 1.0)), (met, sc.metrics)
    for name, key in (("p_after", "p"), ("pm_after", "pm"), ("pv_after", "pv"), ("q_after", "q"), ("qm_after", "qm"), ("qv_after", "qv")):
        idx, val, norm = sc.sampled(name)
        assert _rel(new[key][idx], val) < 1e-12, name
        assert abs(np.linalg.norm(new[key]) - norm) <= 1e-12 * max(norm, 1e-30), name
        assert not np.array_equal(val, fc.sampled(name)[1]), name                      # the second call moved it
    assert _rel(new["d"], sc.duals) < 1e-12
    assert _rel(new["dm"], sc.dm) < 1e-12 and _rel(new["dv"], sc.dv) < 1e-12
    # step 2 is not step 1 again: the twin at step 1 from the same state misses the fixture
    wrong, _, _ = tw.update(st1, fc.LP, fc.LQ, fc.batch, sc.eps_c, sc.eps_a, fc.h, 1, pidx, cidx)
    assert _rel(wrong["d"], sc.duals) > 1e-9 and _rel(wrong["p"][sc.sampled("p_after")[0]], sc.sampled("p_after")[1]) > 1e-9


@pytest.mark.parametrize("c", range(mpo_cases.n_cases()))
def test_reference_quirks_hold_in_the_fixture(c):
    """log_alpha_mean never gets a gradient (alpha_mean is computed from log_alpha_stddev, mpo.py:202): bit-identical after the
    update; the metric alpha_mean equals alpha_std; with the penalty on the improvement weights sum to 2 per row"""
    fc = mpo_cases.load(c)
    A, z, k = fc.A, fc.z, fc.k
    after = z[k + "duals_after"]
    assert after[1:1 + A].tobytes() == fc.state["d"][1:1 + A].tobytes()
    assert np.all(z[k + "duals_exp_avg"][1:1 + A] == 0.0)
    met = z[k + "metrics"]
    assert met[8] == met[9]
    pidx, cidx = (fc.pidx, fc.cidx) if fc.full_obs else (None, None)
    _, _, ex = tw.update(fc.state, fc.LP, fc.LQ, fc.batch, fc.eps_c, fc.eps_a, fc.h, 1, pidx, cidx)
    sums = ex["weights"].sum(0)
    np.testing.assert_allclose(sums, 2.0 if fc.h["action_clipping"] else 1.0, rtol=0, atol=1e-12)
    if not fc.h["action_clipping"]:
        assert met[7] == 0.0 and after[-1] == fc.state["d"][-1]        # no penalty temperature, no step on it


def test_edge_cases_are_exercised():
    """the fixture's cases reach what they are there for"""
    c4 = mpo_cases.load(4)
    after = c4.z[c4.k + "duals_after"]
    assert c4.state["d"][0] == 25.0 and np.all(after[1 + c4.A:1 + 2 * c4.A] == -18.0)      # softplus linear branch; clamp acts
    c3 = mpo_cases.load(3)
    met = c3.z[c3.k + "metrics"]
    assert min(met[12], met[13], met[14]) > c3.h["max_grad_norm"]                          # all three clips act
    assert np.abs(c3.z[c3.k + "act_sample"]).max() > 1.0                  # samples leave [-1, 1]
    c1 = mpo_cases.load(1)
    r = c1.batch[3]
    assert r.max() > c1.h["v_max"] and r.min() < c1.h["v_min"]                            # targets past both edges
    c5 = mpo_cases.load(5)
    assert c5.Op != c5.Oc and c5.Op < c5.O
    c6 = mpo_cases.load(6)         # past the other cases' shapes, an asymmetric support, two calls
    assert (c6.H, c6.NA, c6.A, c6.B, c6.S) == (128, 101, 5, 13, 7) and c6.NA > 64 and c6.B % 4 != 0
    assert c6.h["v_min"] == -20.0 and c6.h["v_max"] == 60.0
    r, d = c6.batch[3], c6.batch[4]
    assert (r > c6.h["v_max"]).any() and (r < c6.h["v_min"]).any() and (d[r > c6.h["v_max"]] == 0).all()
    assert c6.second is not None and mpo_cases.two_call_cases() == [6]
    assert all(mpo_cases.load(c).second is None for c in range(6))
    for c in range(mpo_cases.n_cases()):
        fc = mpo_cases.load(c)
        d, tr, n = fc.batch[4], fc.batch[5], fc.batch[6]
        assert (d * (1 - tr)).sum() > 0 and (tr > 0).any() and sorted(set(n.tolist())) == [1.0, 2.0, 3.0, 4.0]


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference checkout")
def test_fixture_regenerates_bit_for_bit(tmp_path, monkeypatch):
    import importlib.util
    monkeypatch.setenv("RLX_GOLDEN_OUT", str(tmp_path))
    path = os.path.join(os.path.dirname(__file__), "golden", "make_mpo_golden.py")
    spec = importlib.util.spec_from_file_location("make_mpo_golden_t", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        mod.make_mpo()
    finally:
        torch.set_default_dtype(torch.float32)
    za, zb = np.load(mpo_cases.FIXTURE), np.load(os.path.join(str(tmp_path), "mpo_reference.npz"))
    assert sorted(za.files) == sorted(zb.files)
    for k in za.files:
        x, y = za[k], zb[k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


# mpo/pytorch/default_config.py; the plugin differs in compile_mode (nothing is traced) and bf16_mixed_precision_training (fp32),
# and adds threefry_partitionable (its counter RNG)
REFERENCE_DEFAULTS = dict(
    device="gpu", compile_mode="reduce-overhead", bf16_mixed_precision_training=True, total_timesteps=1e9, agent_learning_rate=3e-4,
    dual_learning_rate=1e-2, anneal_agent_learning_rate=False, anneal_dual_learning_rate=False, buffer_size=1e6, learning_starts=5000,
    batch_size=256, actor_update_period=1000, target_network_update_period=100, gamma=0.99, n_steps=4, optimize_every_n_steps=4,
    action_sampling_number=20, max_grad_norm=40.0, epsilon_non_parametric=0.1, epsilon_parametric_mu=0.01, epsilon_parametric_sigma=1e-6,
    epsilon_penalty=0.001, init_log_eta=10.0, init_log_alpha_mean=10.0, init_log_alpha_stddev=1000.0, init_log_penalty_temperature=10.0,
    policy_init_scale=0.5, policy_min_scale=1e-6, action_clipping=True, action_rescaling=True, v_min=-1600.0, v_max=1600.0, nr_atoms=51,
    nr_hidden_units=256, float_epsilon=1e-8, min_log_temperature=-18.0, min_log_alpha=-18.0, enable_observation_normalization=True,
    logging_frequency=300, evaluation_frequency=-1, evaluation_episodes=10)
DIFFERENT = dict(compile_mode="none", bf16_mixed_precision_training=False)


def _reference_config():
    import sys
    import types
    path = os.path.join(REF, "rl_x", "algorithms", "mpo", "pytorch", "default_config.py")
    ml = types.ModuleType("ml_collections")

    class Cfg(dict):
        __getattr__ = dict.__getitem__

        def __setattr__(self, k, v):
            self[k] = v
    ml.config_dict = types.SimpleNamespace(ConfigDict=Cfg)
    saved, ns = sys.modules.get("ml_collections"), {}
    sys.modules["ml_collections"] = ml
    try:
        exec(compile(open(path).read(), path, "exec"), ns)
    finally:
        if saved is None:
            del sys.modules["ml_collections"]
        else:
            sys.modules["ml_collections"] = saved
    ref = dict(ns["get_config"]("mpo.pytorch"))
    ref.pop("name")
    return ref


def test_mpo_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.mpo.hip as plugin
    assert plugin.MPO_HIP == "mpo.hip"
    cfg = am.get_algorithm_config("mpo.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == dict(REFERENCE_DEFAULTS, **DIFFERENT)
    if HAVE_REF:
        assert _reference_config() == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("mpo.hip")
    assert model.__name__ == "MPO"
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert sorted(t.name for t in props.data_interface_types) == ["NUMPY", "TORCH"]


def _config(**alg):
    import types
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.mpo.hip  # noqa: F401
    cfg = am.get_algorithm_config("mpo.hip")
    for k, v in alg.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    return sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
              environment=sn(seed=0, nr_envs=8))


@pytest.mark.parametrize("flags, msg", [(dict(bf16_mixed_precision_training=True), "fp32"), (dict(device="cpu"), "MI355X")])
def test_mpo_hip_refuses_before_any_device_work(flags, msg, monkeypatch):
    import rlx_amd.hip.lib as L
    from rlx_amd.algorithms.mpo.hip.mpo import MPO

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(L.Ctx, "__init__", no_device)
    with pytest.raises(ValueError, match=msg):
        MPO(_config(**flags), None, None, "/nonexistent", None)
