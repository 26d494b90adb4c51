"""CPU: FastTD3's float64 twin (tests/fasttd3_twin.py) against the reference's own outputs (tests/golden/fasttd3_reference.npz:
modules and closures of rl_x/algorithms/fasttd3/pytorch executed in float64), the fixture's provenance, and the `fasttd3.hip`
plugin's registration and flags."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import fasttd3_twin as tw
from oracle.fastsac import clip_grad_norm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FIX = os.path.join(GOLD, "fasttd3_reference.npz")
REF = os.environ.get("RLX_REFERENCE", "/root/reference")
RTOL = 1e-10


def fixture_case(c):
    """-> (z, g, hp, O, A, NA, B, pflat, qflat, clipped); hp as the twin takes it"""
    z = np.load(FIX)
    k = "c%d_" % c
    g = lambda n: z[k + n]
    hp = {n: float(g(n)) for n in ("gamma", "tau", "v_min", "v_max", "learning_rate", "weight_decay", "smoothing_epsilon",
                                   "smoothing_clip_value", "max_grad_norm")}
    O, A, NA, B = int(g("obs_dim")), int(g("act_dim")), int(g("nr_atoms")), int(g("batch"))
    pflat, qflat = tw.make_params(int(g("param_seed")), O, A, NA)
    return z, g, hp, O, A, NA, B, pflat, qflat, bool(int(g("clipped")))


def check_sampled(z, key, full, rtol):
    idx, val, norm = z[key + "_idx"], z[key + "_val"], float(z[key + "_norm"])
    full = np.asarray(full, dtype=np.float64)
    assert np.linalg.norm(full) == pytest.approx(norm, rel=rtol), key
    assert np.linalg.norm(full[idx] - val) <= rtol * np.linalg.norm(val), key


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_twin_acting_matches_the_reference_policy(c):
    z, g, hp, O, A, NA, B, pflat, qflat, clipped = fixture_case(c)
    det, _ = tw.act(pflat, O, A, g("states"), None, None)
    assert _rel(det, g("deterministic_action")) <= RTOL
    low, high = (g("low"), g("high")) if int(g("clip_and_rescale")) else (None, None)
    a, proc = tw.act(pflat, O, A, g("states"), g("act_noise"), g("noise_scales"), low, high)
    assert _rel(a, g("action")) <= RTOL and _rel(proc, g("processed_action")) <= RTOL
    import torch
    for q, name in ((qflat[0], "q1_logits"), (qflat[1], "q2_logits")):
        lg = tw.critic_logits(torch.tensor(q, dtype=torch.float64), O, A, NA, torch.tensor(g("states")), torch.tensor(g("actions")))
        assert _rel(lg.numpy(), g(name)) <= RTOL


@pytest.mark.parametrize("c", [0, 1, 2])
def test_twin_critic_polyak_and_policy_steps_match_the_reference_closures(c):
    z, g, hp, O, A, NA, B, pflat, qflat, clipped = fixture_case(c)
    batch = tuple(g(n) for n in ("states", "next_states", "actions", "rewards", "dones", "truncations", "n_steps"))
    q = np.concatenate(qflat[:2]).astype(np.float64)
    t = np.concatenate(qflat[2:]).astype(np.float64)
    zq = np.zeros_like(q)
    qp, _, _, qt, met, r = tw.critic_update(pflat, q, zq, zq, t, 1, O, A, NA, batch, g("noise_next"), hp, clipped)
    for i, name in enumerate(("q_loss", "q_min", "q_max", "critic_grad_norm")):
        assert met[i] == pytest.approx(float(g(name)), rel=RTOL, abs=1e-12), name
    # the fixture holds the gradients as the optimizer saw them: after clip_grad_norm_
    check_sampled(z, "c%d_gcritic" % c, clip_grad_norm(np.concatenate([r["g_q1"], r["g_q2"]]), hp["max_grad_norm"])[0], RTOL)
    check_sampled(z, "c%d_qparams_after" % c, qp, RTOL)
    check_sampled(z, "c%d_qtarget_after" % c, qt, RTOL)
    zp = np.zeros(pflat.size)
    pp, _, _, pmet, pr = tw.policy_update(pflat, zp, zp, 1, qp, O, A, NA, g("states"), hp, clipped)
    assert pmet[0] == pytest.approx(float(g("policy_loss")), rel=RTOL)
    assert pmet[1] == pytest.approx(float(g("policy_grad_norm")), rel=RTOL)
    check_sampled(z, "c%d_gpolicy" % c, clip_grad_norm(pr["g_policy"], hp["max_grad_norm"])[0], RTOL)
    check_sampled(z, "c%d_pparams_after" % c, pp, RTOL)


def test_fixture_covers_both_clipped_modes_and_active_gradient_clipping():
    z = np.load(FIX)
    assert str(z["source"]).startswith("reference:rl_x/algorithms/fasttd3/pytorch")
    cases = [(int(z["c%d_clipped" % c]), float(z["c%d_max_grad_norm" % c])) for c in range(int(z["n_cases"]))]
    assert (0, -1.0) in cases and (1, -1.0) in cases
    # clipping active: the bar is below both un-clipped norms
    c = [i for i, (_, m) in enumerate(cases) if m > 0][0]
    assert float(z["c%d_critic_grad_norm" % c]) > cases[c][1] and float(z["c%d_policy_grad_norm" % c]) > cases[c][1]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "rl_x")), reason="the reference checkout is not present here")
def test_fasttd3_fixture_regenerates_bit_for_bit(tmp_path):
    env = dict(os.environ, RLX_GOLDEN_OUT=str(tmp_path), RLX_REFERENCE=REF)
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_fasttd3_golden.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    za, zb = np.load(FIX), np.load(os.path.join(str(tmp_path), "fasttd3_reference.npz"))
    assert sorted(za.files) == sorted(zb.files)
    for k in za.files:
        x, y = za[k], zb[k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


# rl_x/algorithms/fasttd3/pytorch/default_config.py:9-38; the plugin differs in device (the only one it runs on), compile_mode
# (nothing is traced) and bf16_mixed_precision_training (fp32), and adds threefry_partitionable (its counter RNG)
REFERENCE_DEFAULTS = dict(
    device="gpu", compile_mode="reduce-overhead", bf16_mixed_precision_training=True, total_timesteps=2000158720, learning_rate=3e-4,
    anneal_learning_rate=False, weight_decay=0.1, batch_size=32768, buffer_size_per_env=10240, learning_starts=10, v_min=-10.0,
    v_max=10.0, tau=0.1, gamma=0.97, nr_atoms=101, n_steps=1, noise_std_min=0.001, noise_std_max=0.4, smoothing_epsilon=0.001,
    smoothing_clip_value=0.5, nr_critic_updates_per_policy_update=2, nr_policy_updates_per_step=1, clipped_double_q_learning=True,
    max_grad_norm=-1.0, action_clipping_and_rescaling=False, enable_observation_normalization=True, logging_frequency=40960,
    evaluation_frequency=-1, save_frequency=4096000)
DIFFERENT = dict(compile_mode="none", bf16_mixed_precision_training=False)


def _reference_file_defaults():
    """the reference's default_config.py executed against a stand-in ml_collections (None where the checkout is absent)"""
    path = os.path.join(REF, "rl_x", "algorithms", "fasttd3", "pytorch", "default_config.py")
    if not os.path.exists(path):
        return None

    class Cfg(dict):
        __getattr__ = dict.__getitem__

        def __setattr__(self, k, v):
            self[k] = v
    ml = types.ModuleType("ml_collections")
    ml.config_dict = types.SimpleNamespace(ConfigDict=Cfg)
    ns = {}
    saved = sys.modules.get("ml_collections")
    sys.modules["ml_collections"] = ml
    try:
        exec(compile(open(path).read(), path, "exec"), ns)
    finally:
        if saved is None:
            del sys.modules["ml_collections"]
        else:
            sys.modules["ml_collections"] = saved
    cfg = dict(ns["get_config"]("fasttd3.pytorch"))
    cfg.pop("name")
    return cfg


def test_fasttd3_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.fasttd3.hip as plugin
    assert plugin.FASTTD3_HIP == "fasttd3.hip"
    cfg = am.get_algorithm_config("fasttd3.hip")
    assert cfg.name == "fasttd3.hip"
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == dict(REFERENCE_DEFAULTS, **DIFFERENT)
    ref = _reference_file_defaults()
    if ref is not None:
        assert ref == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("fasttd3.hip")
    assert model.__name__ == "FastTD3"
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.observation_space_types] == ["FLAT_VALUES"]


def _config(**alg):
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.fasttd3.hip  # noqa: F401
    cfg = am.get_algorithm_config("fasttd3.hip")
    for k, v in alg.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    return sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
              environment=sn(seed=0, nr_envs=8))


@pytest.mark.parametrize("flags, msg", [(dict(bf16_mixed_precision_training=True), "fp32"), (dict(device="cpu"), "MI355X"),
                                        (dict(max_grad_norm=0.0), "max_grad_norm")])
def test_fasttd3_hip_refuses_what_it_does_not_emulate(flags, msg):
    from rlx_amd.algorithms.fasttd3.hip.fasttd3 import FastTD3
    with pytest.raises(ValueError, match=msg):
        FastTD3(_config(**flags), None, None, "/nonexistent", None)


def test_relu_descriptor_layout_matches_the_twin():
    from rlx_amd.hip import relu_mlp_desc, ACT_RELU
    d = relu_mlp_desc(60, tw.CRITIC_HIDDEN, 101)
    assert (d.in_dim, d.n_hidden, list(d.hidden)[:3], d.out_dim, d.act, d.ln_first, d.has_logstd) == (60, 3, [1024, 512, 256], 101, ACT_RELU, 0, 0)
    p, q = tw.make_params(0, 48, 12, 101)
    assert p.size == tw.param_count(48, tw.POLICY_HIDDEN, 12) and q[0].size == tw.param_count(60, tw.CRITIC_HIDDEN, 101)
