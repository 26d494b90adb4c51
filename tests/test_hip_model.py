"""CPU: the host layer the five net_pass plugins share (rlx_amd/algorithms/hip_model.py): the refusals come before any device work
with their texts unchanged, the merged initialiser draws what its two earlier forms drew, the shared checkpoint round-trips, and
the module-level observation_indices is what PPO._observation_indices was."""
import os
import re
import types

import numpy as np
import pytest
import torch

from rlx_amd.algorithms import hip_model as hm

PLUGINS = {"fastsac.hip": "FastSAC", "fasttd3.hip": "FastTD3", "mpo.hip": "MPO", "fastmpo.hip": "FastMPO", "reppo.hip": "REPPO"}
DEVICE = "{} runs on MI355X only: --algorithm.device must be 'gpu' (no CPU fallback)"
BF16 = "{} computes in fp32: set --algorithm.bf16_mixed_precision_training=False"
INTERFACE = "{} needs a TORCH data-interface environment"
REFUSALS = [(name, dict(device="cpu"), "TORCH", DEVICE) for name in PLUGINS]
REFUSALS += [(name, dict(bf16_mixed_precision_training=True), "TORCH", BF16) for name in PLUGINS if name != "fastmpo.hip"]   # it has no such flag
REFUSALS += [(name, dict(), "NUMPY", INTERFACE) for name in PLUGINS if name != "mpo.hip"]                                      # it takes both


def _plugin(name, **flags):
    import importlib
    from rlx_amd.algorithms import algorithm_manager as am
    importlib.import_module("rlx_amd.algorithms." + name)
    cfg = am.get_algorithm_config(name)
    for k, v in flags.items():
        assert k in cfg, k
        cfg[k] = v
    sn = types.SimpleNamespace
    config = sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
                environment=sn(seed=0, nr_envs=8))
    return am.get_algorithm_model_class(name), config


def _env(interface):
    from rlx_amd.environments.data_interface_type import DataInterfaceType
    return types.SimpleNamespace(general_properties=types.SimpleNamespace(data_interface_type=DataInterfaceType[interface]))


@pytest.mark.parametrize("name, flags, interface, text", REFUSALS)
def test_plugins_refuse_before_any_device_work(name, flags, interface, text, monkeypatch):
    import rlx_amd.hip.lib as L

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(L.Ctx, "__init__", no_device)
    cls, config = _plugin(name, **flags)
    assert cls.__name__ == PLUGINS[name] and cls._NAME == name
    with pytest.raises(ValueError, match="^" + re.escape(text.format(name)) + "$"):
        cls(config, _env(interface), None, "/nonexistent", None)


# ------------------------------------------------------------------------------------------------------------- the initialiser
def _fastsac_form(rng, in_dim, hidden, out_dim, zero_head):
    """fastsac.py's initialiser before the merge, kept as the reference"""
    parts, d = [], in_dim
    for h in hidden:
        bound = 1.0 / np.sqrt(d)
        parts += [rng.uniform(-bound, bound, (d, h)), rng.uniform(-bound, bound, h), np.ones(h), np.zeros(h)]
        d = h
    bound = 0.0 if zero_head else 1.0 / np.sqrt(d)
    parts += [rng.uniform(-bound, bound, (d, out_dim)) if bound else np.zeros((d, out_dim)),
              rng.uniform(-bound, bound, out_dim) if bound else np.zeros(out_dim)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def _fasttd3_form(rng, in_dim, hidden, out_dim, head_std=None):
    """fasttd3.py's initialiser before the merge, kept as the reference"""
    parts, d = [], in_dim
    for li, h in enumerate(list(hidden) + [out_dim]):
        bound = 1.0 / np.sqrt(d)
        if li == len(hidden) and head_std is not None:
            parts += [rng.normal(0.0, head_std, (d, h)), np.zeros(h)]
        else:
            parts += [rng.uniform(-bound, bound, (d, h)), rng.uniform(-bound, bound, h)]
        d = h
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


@pytest.mark.parametrize("layer_norm, head_std, reference", [
    (True, None, lambda rng: _fastsac_form(rng, 5, (8, 4), 3, False)), (False, None, lambda rng: _fasttd3_form(rng, 5, (8, 4), 3)),
    (True, 0, lambda rng: _fastsac_form(rng, 5, (8, 4), 3, True)), (False, 0.01, lambda rng: _fasttd3_form(rng, 5, (8, 4), 3, 0.01))])
def test_merged_initialiser_draws_what_the_two_forms_drew(layer_norm, head_std, reference):
    got_rng, ref_rng = np.random.default_rng(7), np.random.default_rng(7)
    for _ in range(2):                  # the second call continues the stream: the critics follow the policy on one rng
        got, ref = hm.torch_linear_flat(got_rng, 5, (8, 4), 3, layer_norm, head_std=head_std), reference(ref_rng)
        assert got.dtype == np.float32 and got.size == 5 * 8 + 8 * 4 + 4 * 3 + 15 + (24 if layer_norm else 0)
        assert np.array_equal(got, ref)
    assert got_rng.random() == ref_rng.random()            # and leaves it where the earlier form left it


# ------------------------------------------------------------------------------------------------------------- the checkpoint
class _Dummy(hm.HipModel):
    _NAME = "dummy.hip"
    _FILE = "dummy.model"
    _STATE = ("weights", "moments")
    _COUNTERS = ("steps", "opt_counts")

    def __init__(self, config, train_env, eval_env, run_path, writer):
        self.torch, self.device, self.config = torch, torch.device("cpu"), config
        self.save_path = os.path.join(run_path, "models")
        self.obs_norm = bool(config.algorithm.enable_observation_normalization)
        self.weights, self.moments = torch.zeros(3, 2), torch.zeros(5)
        self.norm_mean, self.norm_var, self.norm_std = torch.zeros(4), torch.ones(4), torch.ones(4)
        self.norm_count = torch.zeros(1, dtype=torch.int64)
        self.steps, self.opt_counts, self.key = 0, (0, 0, 0), np.zeros(2, np.uint32)
        self.copy = None

    def _after_load(self):
        self.copy = self.weights.clone()


@pytest.mark.parametrize("obs_norm", [False, True])
def test_shared_checkpoint_round_trip(tmp_path, obs_norm):
    from rlx_amd.plugin import flag_namespace
    sn = types.SimpleNamespace
    config = sn(algorithm=flag_namespace("dummy.hip", dict(enable_observation_normalization=obs_norm, gamma=0.5)), runner=sn())
    os.makedirs(tmp_path / "models")
    m = _Dummy(config, None, None, str(tmp_path), None)
    m.weights, m.moments = torch.arange(6.0).reshape(3, 2), torch.linspace(-1.0, 1.0, 5)
    m.norm_mean, m.norm_count[0] = torch.full((4,), 0.25), 2 ** 40
    m.steps, m.opt_counts, m.key = 12, (7, 3, 2 ** 33), np.array([4000000000, 5], np.uint32)
    m.save()
    path = os.path.join(m.save_path, "dummy.model")
    assert os.listdir(m.save_path) == ["dummy.model"]                          # written to a temporary name, then replaced
    ckpt = np.load(path, allow_pickle=False)
    norm = hm.HipModel._NORM_STATE if obs_norm else ()
    assert set(ckpt.files) == set(_Dummy._STATE + _Dummy._COUNTERS + norm + ("key", "config_algorithm"))
    assert ckpt["steps"].shape == () and ckpt["opt_counts"].dtype == np.int64 and ckpt["weights"].dtype == np.float32
    assert not obs_norm or ckpt["norm_count"].dtype == np.int64
    config2 = sn(algorithm=flag_namespace("dummy.hip", dict(enable_observation_normalization=obs_norm, gamma=0.9)), runner=sn(load_model=path))
    m2 = _Dummy.load(config2, None, None, str(tmp_path), None, [])
    assert isinstance(m2, _Dummy) and config2.algorithm.gamma == 0.5           # adopt_checkpoint_config: the stored flag wins
    assert torch.equal(m2.weights, m.weights) and torch.equal(m2.moments, m.moments) and torch.equal(m2.copy, m.weights)
    assert (m2.steps, m2.opt_counts) == (12, (7, 3, 2 ** 33)) and type(m2.steps) is int and type(m2.opt_counts[2]) is int
    assert m2.key.dtype == np.uint32 and np.array_equal(m2.key, m.key)
    assert torch.equal(m2.norm_mean, m.norm_mean if obs_norm else torch.zeros(4))     # the normaliser only when it is on
    assert int(m2.norm_count) == (2 ** 40 if obs_norm else 0)
    config3 = sn(algorithm=flag_namespace("dummy.hip", dict(enable_observation_normalization=obs_norm, gamma=0.9)), runner=sn(load_model=path))
    _Dummy.load(config3, None, None, str(tmp_path), None, ["algorithm.gamma"])
    assert config3.algorithm.gamma == 0.9                                      # ... unless the flag was given on the command line


# ------------------------------------------------------------------------------------------------------------- observation indices
def test_observation_indices_is_what_ppo_had():
    from rlx_amd.algorithms.ppo.hip.ppo import PPO
    sn = types.SimpleNamespace
    for fn in (hm.observation_indices, PPO._observation_indices):
        assert fn(sn(), 6) == (None, None)
        p, c = fn(sn(policy_observation_indices=[4, 1, 2]), 6)                 # policy only: the critic reads every column
        assert p.dtype == c.dtype == np.int32 and p.tolist() == [4, 1, 2] and c.tolist() == [0, 1, 2, 3, 4, 5]
        p, c = fn(sn(policy_observation_indices=None, critic_observation_indices=np.array([[0, 5]])), 6)
        assert p.tolist() == [0, 1, 2, 3, 4, 5] and c.tolist() == [0, 5]
        for bad in ([6], [-1, 2], []):
            with pytest.raises(ValueError, match=re.escape("critic_observation_indices must be non-empty and within [0, 6)")):
                fn(sn(critic_observation_indices=bad), 6)
    assert PPO._observation_indices is hm.observation_indices
