"""GPU: tqc.hip through the Runner on the Humanoid-shaped synthetic env (tests/test_gpu_train.py::test_sac_runner_train's sizes),
a run at ensemble 5, and the checkpoint round trip."""
import copy
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _train(monkeypatch, total, *extra):
    """-> (model, every record the metric sink was given)"""
    from rlx_amd.plugin import MetricSink
    from rlx_amd.runner.runner import Runner
    records = []
    write = MetricSink.write

    def recording_write(self, step, metrics):
        records.append(dict(metrics))
        return write(self, step, metrics)

    monkeypatch.setattr(MetricSink, "write", recording_write)
    monkeypatch.setattr(sys, "argv", ["experiment.py", "--algorithm.name=tqc.hip", "--environment.name=synthetic.random_obs",
                                      "--runner.mode=train", "--environment.nr_envs=64", "--environment.obs_dim=376",
                                      "--environment.act_dim=17", "--environment.horizon=50",
                                      "--algorithm.batch_size=256", "--algorithm.buffer_size=64000",
                                      "--algorithm.learning_starts=640", f"--algorithm.total_timesteps={total}",
                                      "--algorithm.logging_frequency=6400", *extra])
    return Runner().run(), records


def test_tqc_runner_train(monkeypatch, tmp_path):
    """runs, counts, finite metrics, alpha adapts, the quantile loss falls; evaluation runs; a checkpoint restores every tensor,
    counter, key and generator state, and the next update of the restored model is bit-identical"""
    model, records = _train(monkeypatch, 19200)
    m = model.last_metrics
    assert m["steps/nr_env_steps"] == 19200 and m["steps/nr_updates"] == 290 and model.opt_count == 290
    for k, v in m.items():
        assert np.isfinite(v), k
    assert m["entropy/alpha"] < 1.0          # entropy above target -> alpha decreases
    first = next(r for r in records if "loss/q_loss" in r)
    print("tqc.hip q_loss: first interval %.4f, last %.4f" % (first["loss/q_loss"], m["loss/q_loss"]))
    assert np.isfinite(m["loss/q_loss"]) and m["loss/q_loss"] < first["loss/q_loss"]
    assert model.size == min(300, model.capacity)
    assert model.qparams.numel() == 2 * model.nq and model.qdesc.out_dim == 25
    assert len(model.test(2)) == 2
    # ---- checkpoint round trip
    model.save_path = str(tmp_path)
    path = model.save()
    config = copy.deepcopy(model.config)
    config.runner.load_model = path
    loaded = type(model).load(config, model.train_env, model.eval_env, str(tmp_path), None, [])
    for k in model._STATE:
        assert torch.equal(getattr(model, k), getattr(loaded, k)), k
    assert loaded.opt_count == model.opt_count == 290 and np.array_equal(loaded.key, model.key) and loaded.key.dtype == np.uint32
    assert loaded.rng.bit_generator.state == model.consumed_rng_state()
    assert (loaded.ensemble_size, loaded.nr_atoms_per_net, loaded.nq) == (model.ensemble_size, model.nr_atoms_per_net, model.nq)
    loaded._alloc()
    g = torch.Generator(device=model.device)
    g.manual_seed(5)
    f = dict(device=model.device, generator=g)
    batch = (torch.randn(256, 376, **f), torch.randn(256, 376, **f), torch.tanh(torch.randn(256, 17, **f)), torch.randn(256, **f),
             (torch.rand(256, **f) < 0.2).float())
    model.update(batch)
    loaded.update(batch)
    for k in model._STATE:
        assert torch.equal(getattr(model, k), getattr(loaded, k)), k
    assert torch.equal(model.metrics_dev, loaded.metrics_dev) and np.array_equal(loaded.key, model.key) and loaded.opt_count == 291


def test_tqc_runner_train_five_critics(monkeypatch):
    model, _ = _train(monkeypatch, 1280, "--algorithm.ensemble_size=5")
    m = model.last_metrics
    assert m["steps/nr_env_steps"] == 1280 and m["steps/nr_updates"] == 10 and model.opt_count == 10
    for k, v in m.items():
        assert np.isfinite(v), k
    assert model.qparams.numel() == 5 * model.nq and model.nr_total_atoms == 125 and model.nr_target_atoms == 115
