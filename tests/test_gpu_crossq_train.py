"""GPU: crossq.hip through the Runner on the synthetic env -- two batch-renormalised critics, no target networks, the policy updated
when global_step % policy_delay == 0, the r / d correction switching on after 10 updates -- and the checkpoint round trip."""
import copy
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, DELAY = 64, 3


def _train(monkeypatch, total, *extra):
    from rlx_amd.runner.runner import Runner
    monkeypatch.setattr(sys, "argv", ["experiment.py", "--algorithm.name=crossq.hip", "--environment.name=synthetic.random_obs",
                                      "--runner.mode=train", "--environment.nr_envs=16", "--environment.obs_dim=24",
                                      "--environment.act_dim=4", "--environment.horizon=20", "--algorithm.ensemble_size=2",
                                      f"--algorithm.policy_delay={DELAY}", "--algorithm.batch_renorm_warmup_steps=10",
                                      f"--algorithm.batch_size={B}", "--algorithm.policy_nr_hidden_units=64",
                                      "--algorithm.critic_nr_hidden_units=128", "--algorithm.buffer_size=3200",
                                      "--algorithm.learning_starts=64", f"--algorithm.total_timesteps={total}",
                                      "--algorithm.logging_frequency=320", *extra])
    return Runner().run()


def _batch(model, seed):
    g = torch.Generator(device=model.device)
    g.manual_seed(seed)
    f = dict(device=model.device, generator=g)
    return (torch.randn(B, 24, **f), torch.randn(B, 24, **f), torch.tanh(torch.randn(B, 4, **f)), torch.randn(B, **f),
            (torch.rand(B, **f) < 0.2).float())


def test_crossq_runner_train_and_checkpoint(monkeypatch, tmp_path):
    """40 env steps of 16 envs, 36 critic updates: finite metrics, the policy updated exactly where global_step % 3 == 0 (12 times),
    both statistics vectors moved; then save -> load -> one more update of both models gives the bits of the uninterrupted run"""
    model = _train(monkeypatch, 640)
    m = model.last_metrics
    assert m["steps/nr_env_steps"] == 640 and m["steps/nr_updates"] == 36 and model.global_step == 640
    due = sum(1 for g in range(16, 641, 16) if g > 64 and g % DELAY == 0)
    assert due == 12 and model.nr_q_updates == 36 and model.nr_policy_updates == due and model.opt_count == due
    for k, v in m.items():
        assert np.isfinite(v), k
    for k in model._STATE:
        assert torch.isfinite(getattr(model, k)).all(), k
    assert type(model).__name__ == "CrossQ" and not hasattr(model, "qtarget") and not hasattr(model, "tau")
    # per critic: BRN over the 28 inputs, Dense 28 -> 128, BRN, Dense 128 -> 128, BRN, head; statistics for 28 + 128 + 128 columns
    assert model.nq == (2 * 28 + 28 * 128 + 128) + (2 * 128 + 128 * 128 + 128) + (2 * 128 + 128 + 1)
    assert model.qparams.numel() == 2 * model.nq and model.qstats.numel() == 2 * 2 * (28 + 128 + 128) and model.pstats.numel() == 2 * (24 + 64 + 64)
    assert model.critic_layout()["batch_renorm"]["statistics_per_net"] == 2 * (28 + 128 + 128)
    fresh = torch.cat([torch.zeros(28), torch.ones(28)]).to(model.device)
    assert not torch.equal(model.qstats[:56], fresh) and not torch.equal(model.pstats[:48], torch.cat([torch.zeros(24), torch.ones(24)]).to(model.device))
    assert not torch.equal(model.qparams[:56], fresh) and model.log_alpha.item() != 0.0            # the first BRN's scale and bias trained
    key_before = model.key.copy()
    assert len(model.test(2)) == 2 and np.array_equal(model.key, key_before)
    # ---- checkpoint round trip
    model.save_path = str(tmp_path)
    path = model.save()
    config = copy.deepcopy(model.config)
    config.runner.load_model = path
    loaded = type(model).load(config, model.train_env, model.eval_env, str(tmp_path), None, [])
    for k in model._STATE:
        assert torch.equal(getattr(model, k), getattr(loaded, k)), k
    assert (loaded.nr_q_updates, loaded.nr_policy_updates, loaded.global_step) == (36, 12, 640)
    assert np.array_equal(loaded.key, model.key) and loaded.key.dtype == np.uint32
    assert loaded.rng.bit_generator.state == model.consumed_rng_state()
    assert loaded.critic_layout() == model.critic_layout()
    loaded._alloc()
    batch = _batch(model, 5)
    for mdl in (model, loaded):
        mdl.update(batch, policy=True)
    for k in model._STATE:
        assert torch.equal(getattr(model, k), getattr(loaded, k)), k
    assert torch.equal(model.metrics_dev, loaded.metrics_dev) and np.array_equal(loaded.key, model.key)
    assert (loaded.nr_q_updates, loaded.nr_policy_updates) == (37, 13)
    # ---- another critic width does not take this checkpoint
    config.algorithm.critic_nr_hidden_units = 64
    with pytest.raises(ValueError, match="crossq.hip: the checkpoint's critic layout"):
        type(model).load(config, model.train_env, model.eval_env, str(tmp_path), None, ["algorithm.critic_nr_hidden_units"])
