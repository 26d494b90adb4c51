"""GPU: droq.hip through the Runner on the synthetic env -- two Dropout -> LayerNorm -> ReLU critics, both in the target minimum, two
critic steps per policy step, dropout rate 0.1 -- and the checkpoint round trip."""
import copy
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G, B = 2, 64


def _train(monkeypatch, total, *extra):
    from rlx_amd.runner.runner import Runner
    monkeypatch.setattr(sys, "argv", ["experiment.py", "--algorithm.name=droq.hip", "--environment.name=synthetic.random_obs",
                                      "--runner.mode=train", "--environment.nr_envs=16", "--environment.obs_dim=24",
                                      "--environment.act_dim=4", "--environment.horizon=20",
                                      "--algorithm.ensemble_size=2", "--algorithm.in_target_minimization_size=2", "--algorithm.dropout_rate=0.1",
                                      f"--algorithm.q_update_steps={G}", f"--algorithm.batch_size={B}", "--algorithm.nr_hidden_units=64",
                                      "--algorithm.buffer_size=3200", "--algorithm.learning_starts=64",
                                      f"--algorithm.total_timesteps={total}", "--algorithm.logging_frequency=320", *extra])
    return Runner().run()


def _batch(model, seed):
    g = torch.Generator(device=model.device)
    g.manual_seed(seed)
    f = dict(device=model.device, generator=g)
    n = G * B
    return (torch.randn(n, 24, **f), torch.randn(n, 24, **f), torch.tanh(torch.randn(n, 4, **f)), torch.randn(n, **f),
            (torch.rand(n, **f) < 0.2).float())


def test_droq_runner_train_and_checkpoint(monkeypatch, tmp_path):
    """40 env steps of 16 envs, 36 updates: finite metrics, two critic steps per policy step, q_update_steps batches per sample; then
    save -> load -> one more update gives the bits of the uninterrupted run (the masks come from the restored key), and a checkpoint is
    refused when dropout_rate differs"""
    model = _train(monkeypatch, 640)
    m = model.last_metrics
    assert m["steps/nr_env_steps"] == 640 and m["steps/nr_updates"] == 36
    assert model.nr_policy_updates == 36 and model.nr_q_updates == 2 * model.nr_policy_updates and model.opt_count == 36
    for k, v in m.items():
        assert np.isfinite(v), k
    assert torch.isfinite(model.metrics_dev).all() and torch.isfinite(model.qparams).all() and torch.isfinite(model.pparams).all()
    assert type(model).__name__ == "DroQ" and model.critic_layout()["layer_norm"] is True and model.critic_layout()["dropout_rate"] == 0.1
    # per critic: two hidden blocks of W, b, LayerNorm scale, LayerNorm bias, then the head
    assert model.nq == (28 * 64 + 3 * 64) + (64 * 64 + 3 * 64) + 64 + 1
    assert model.qparams.numel() == 2 * model.nq and model.qdesc.out_dim == 1 and model.batch[0].shape == (G * B, 24)
    ln = slice(28 * 64 + 64, 28 * 64 + 3 * 64)                    # the first block's scale and bias: trained away from (1, 0)
    assert not torch.equal(model.qparams[ln], torch.cat([torch.ones(64), torch.zeros(64)]).to(model.qparams.device))
    assert not torch.equal(model.qparams, model.qtarget) and model.log_alpha.item() != 0.0
    assert len(model.test(2)) == 2
    # ---- checkpoint round trip
    model.save_path = str(tmp_path)
    path = model.save()
    config = copy.deepcopy(model.config)
    config.runner.load_model = path
    loaded = type(model).load(config, model.train_env, model.eval_env, str(tmp_path), None, [])
    for k in model._STATE:
        assert torch.equal(getattr(model, k), getattr(loaded, k)), k
    assert (loaded.nr_q_updates, loaded.nr_policy_updates) == (72, 36)
    assert np.array_equal(loaded.key, model.key) and loaded.key.dtype == np.uint32
    assert loaded.rng.bit_generator.state == model.consumed_rng_state()
    assert loaded.critic_layout() == model.critic_layout()
    loaded._alloc()
    batch = _batch(model, 5)
    model.update(batch)
    loaded.update(batch)
    for k in model._STATE:
        assert torch.equal(getattr(model, k), getattr(loaded, k)), k
    assert torch.equal(model.metrics_dev, loaded.metrics_dev) and np.array_equal(loaded.key, model.key)
    assert (loaded.nr_q_updates, loaded.nr_policy_updates) == (74, 37)
    # ---- another dropout rate does not take this checkpoint
    config.algorithm.dropout_rate = 0.2
    with pytest.raises(ValueError, match="droq.hip: the checkpoint's critic layout"):
        type(model).load(config, model.train_env, model.eval_env, str(tmp_path), None, ["algorithm.dropout_rate"])
