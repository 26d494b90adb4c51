"""CPU: the float64 numpy ESPO twin (tests/espo_twin.py) against the reference fixture (tests/golden/espo_reference.npz, outputs of
the reference's own modules and closures), the conditions the fixture's cases were generated under, the library's export and
binding, and the plugin's registration and refusals."""
import ctypes
import os
import types

import numpy as np
import pytest

import espo_cases as ec
import espo_twin as tw

GOLD = os.path.dirname(ec.FIXTURE)


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


def test_fixture_is_inputs_and_outputs_only():
    z = ec.fixture()
    assert str(z["source"]).startswith("reference:rl_x/algorithms/espo/pytorch")
    assert os.path.getsize(ec.FIXTURE) < os.path.getsize(os.path.join(GOLD, "mpo_reference.npz")) // 2
    for k in z.files:
        assert z[k].dtype.kind in "fiuU", (k, z[k].dtype)          # numbers and two strings: nothing that could hold code
    assert int(z["n_cases"]) == 8


@pytest.mark.parametrize("c", range(ec.n_cases()))
def test_twin_reproduces_the_reference_fixture(c):
    fc = ec.load(c)
    z, k = fc.z, fc.k
    # Policy.get_logprob_entropy / get_deterministic_action (policy.py:57-73) and GAE (espo.py:112-120)
    lp, ent, _ = tw.logprob_entropy(fc.p0, fc.LP, fc.states[:, fc.pidx], fc.actions)
    assert _rel(lp, z[k + "logprob0"]) < 1e-12 and _rel(ent, z[k + "entropy0"]) < 1e-12
    assert _rel(tw.deterministic_action(fc.p0, fc.LP, fc.states[:, fc.pidx], fc.low, fc.high), z[k + "det_action0"]) < 1e-12
    adv, ret = tw.gae(z[k + "rewards"], z[k + "terminations"], z[k + "values"], z[k + "next_values"], fc.h["gamma"], fc.h["gae_lambda"])
    assert _rel(adv, z[k + "gae_advantages"]) < 1e-12 and _rel(ret, z[k + "gae_returns"]) < 1e-12
    assert np.array_equal(adv.reshape(-1).astype(np.float32), fc.advantages.astype(np.float32))
    # the stored rows are the reference's draws
    assert np.array_equal(tw.draw_indices(np.random.default_rng(int(z[k + "param_seed"])), fc.B, fc.mb, fc.E), fc.idx)
    # the epoch loop with its stop
    st, met, run, info = fc.twin()
    assert run == fc.epochs_run == (fc.E if fc.stop_epoch < 0 else fc.stop_epoch + 1) and st["count"] == run
    assert met.shape == fc.metrics.shape == (run, 7)
    assert np.all(np.abs(met - fc.metrics) <= 1e-12 * np.maximum(np.abs(fc.metrics), 1.0)), (met, fc.metrics)
    for name, key in (("p_after", "p"), ("pm_after", "pm"), ("pv_after", "pv"), ("c_after", "c"), ("cm_after", "cm"), ("cv_after", "cv")):
        idx, val, norm = fc.sampled(name)
        assert _rel(st[key][idx], val) < 1e-12, name
        assert abs(np.linalg.norm(st[key]) - norm) <= 1e-12 * max(norm, 1e-30), name
    assert ec.margins_ok(info)


def test_cases_reach_what_they_are_there_for():
    runs = [ec.load(c).epochs_run for c in range(8)]
    assert runs == [6, 4, 3, 4, 6, 6, 1, 6]
    assert [ec.load(c).h["delta_calc_operator"] for c in (2, 3)] == ["median", "median"] and ec.load(2).mb % 2 == 0 and ec.load(3).mb == 15
    c4 = ec.load(4)
    assert c4.h["entropy_coef"] == 0.01 and np.all(c4.metrics[:, 5] > 10 * c4.h["max_grad_norm"]) and np.all(c4.metrics[:, 6] > 10 * 1e-3)
    c5 = ec.load(5)
    assert (len(c5.pidx), len(c5.cidx), c5.O) == (6, 10, 12) and not c5.full_obs
    c6 = ec.load(6)
    assert (c6.O, c6.A, c6.H, c6.mb) == (10, 5, 128, 13)
    c7 = ec.load(7)
    assert c7.stop_epoch == c7.E - 1 and c7.metrics[-1, 3] > c7.h["max_ratio_delta"] and np.all(c7.metrics[:-1, 3] < c7.h["max_ratio_delta"])


def test_stop_applies_the_tripping_epoch_in_full_and_nothing_after():
    """espo.py:277: the break comes after both steps of the epoch.  A run that stops after epoch k equals a run of k + 1 epochs with
    no threshold; one more epoch moves the parameters on."""
    fc = ec.load(1)
    k = fc.stop_epoch
    st, met, run, _ = fc.twin()
    ref, met2, run2, _ = fc.twin(max_epochs=k + 1, max_ratio_delta=np.inf)
    assert run == run2 == k + 1 and np.array_equal(met, met2)
    assert all(np.array_equal(st[n], ref[n]) for n in ("p", "pm", "pv", "c", "cm", "cv"))
    more, _, run3, _ = fc.twin(max_epochs=k + 2, max_ratio_delta=np.inf)
    assert run3 == k + 2 and not np.array_equal(more["p"], st["p"]) and not np.array_equal(more["c"], st["c"])


def test_lower_median_and_nan():
    assert tw.lower_median(np.array([4.0, 1.0, 3.0, 2.0])) == 2.0 and tw.lower_median(np.array([5.0, 1.0, 3.0])) == 3.0
    assert np.isnan(tw.lower_median(np.array([1.0, np.nan, 0.5])))
    import torch
    x = torch.tensor([4.0, 1.0, 3.0, 2.0], dtype=torch.float64)
    assert float(torch.median(x)) == 2.0 and abs(float(x.std()) - np.std(x.numpy(), ddof=1)) < 1e-15


def test_library_exports_and_binds_the_update():
    from rlx_amd.hip import EspoHparams
    from rlx_amd.hip import lib as L
    assert "rlx_espo_update_f32" in L.EXPORTED_SYMBOLS
    lib = L.load_library()
    assert lib.rlx_espo_update_f32.argtypes[-1] is ctypes.c_void_p and len(lib.rlx_espo_update_f32.argtypes) == 29
    assert ctypes.sizeof(EspoHparams) == 8 * 4                      # include/rlx_hip.h: seven floats and delta_op
    assert hasattr(L.Ctx, "espo_update")
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "rlx_hip.h")).read()
    assert "int rlx_espo_update_f32(" in header and "espo.py:236-278" in header
    # the flat layout is rlx_mlp_param_count's
    from rlx_amd.hip import ACT_TANH, mlp_desc
    LP, LC = tw.layout(48, 256, 12, True), tw.layout(48, 256, 1, False)
    assert lib.rlx_mlp_param_count(ctypes.byref(mlp_desc(48, [256, 256], 12, ACT_TANH, False, True))) == LP["n"]
    assert lib.rlx_mlp_param_count(ctypes.byref(mlp_desc(48, [256, 256], 1, ACT_TANH, False, False))) == LC["n"]


REFERENCE_DEFAULTS = dict(
    device="gpu", compile_mode="reduce-overhead", bf16_mixed_precision_training=True, total_timesteps=1e9, learning_rate=3e-4,
    anneal_learning_rate=False, nr_steps=2048, max_epochs=300, minibatch_size=64, gamma=0.99, gae_lambda=0.95, max_ratio_delta=0.25,
    delta_calc_operator="mean", entropy_coef=0.0, critic_coef=0.5, max_grad_norm=0.5, std_dev=1.0, action_clipping_and_rescaling=True,
    nr_hidden_units=256, evaluation_frequency=-1, evaluation_episodes=10)      # espo/pytorch/default_config.py:7-29
DIFFERENT = dict(compile_mode="none", bf16_mixed_precision_training=False)


def test_espo_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.espo.hip as plugin
    assert plugin.ESPO_HIP == "espo.hip"
    cfg = am.get_algorithm_config("espo.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True and got.pop("fused_rollout") is True
    assert got == dict(REFERENCE_DEFAULTS, **DIFFERENT)
    model = am.get_algorithm_model_class("espo.hip")
    assert model.__name__ == "ESPO"
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


def test_runner_resolves_espo_hip():
    from rlx_amd.algorithms import algorithm_manager as am
    from rlx_amd.runner.runner import Runner
    assert Runner._import_plugin("algorithms", "espo.hip", ["rlx_amd"]) == "rlx_amd"
    assert am.get_algorithm_general_properties("espo.hip") is am.get_algorithm_model_class("espo.hip").general_properties()


def _config(**alg):
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.espo.hip  # noqa: F401
    cfg = am.get_algorithm_config("espo.hip")
    for k, v in alg.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    return sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
              environment=sn(seed=0, nr_envs=8))


def _env(interface):
    from rlx_amd.environments.data_interface_type import DataInterfaceType
    return types.SimpleNamespace(general_properties=types.SimpleNamespace(data_interface_type=DataInterfaceType[interface]))


@pytest.mark.parametrize("flags, interface, msg", [
    (dict(bf16_mixed_precision_training=True), "TORCH", "fp32"), (dict(device="cpu"), "TORCH", "MI355X"),
    (dict(delta_calc_operator="max"), "TORCH", "Unknown delta_calc_operator"), (dict(), "NUMPY", "TORCH data-interface"),
    (dict(minibatch_size=1), "TORCH", "minibatch_size"), (dict(minibatch_size=8192), "TORCH", "minibatch_size"),
    (dict(minibatch_size=64, nr_steps=4), "TORCH", "minibatch_size"), (dict(max_epochs=0), "TORCH", "max_epochs")])
def test_espo_hip_refuses_before_any_device_work(flags, interface, msg, monkeypatch):
    import rlx_amd.hip.lib as L
    from rlx_amd.algorithms.espo.hip.espo import ESPO

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(L.Ctx, "__init__", no_device)
    with pytest.raises(ValueError, match=msg):
        ESPO(_config(**flags), _env(interface), None, "/nonexistent", None)


def test_espo_hip_refuses_more_than_one_rank(monkeypatch):
    import torch.distributed as dist
    import rlx_amd.hip.lib as L
    from rlx_amd.algorithms.espo.hip.espo import ESPO
    monkeypatch.setattr(L.Ctx, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work before the refusal")))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(ValueError, match="one GPU"):
        ESPO(_config(), _env("TORCH"), None, "/nonexistent", None)
