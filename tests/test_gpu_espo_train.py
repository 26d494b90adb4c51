"""GPU: `espo.hip` end to end through the reference-style entry point (Runner -> registry -> espo.hip on synthetic.random_obs): the
loop runs, metrics are finite, the epoch bookkeeping follows the reference (espo.py:288-294), the synthetic task is learnt, and a
checkpoint continues where it was saved."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_EPOCHS = 24


def _run(monkeypatch, *flags):
    from rlx_amd.runner.runner import Runner
    monkeypatch.setattr(sys, "argv", ["experiment.py", "--algorithm.name=espo.hip", "--environment.name=synthetic.random_obs",
                                      "--runner.mode=train", *flags])
    return Runner().run()


def test_runner_train_learns(monkeypatch):
    iters, N, T = 40, 256, 32
    seen = []
    from rlx_amd.algorithms.espo.hip.espo import ESPO
    update = ESPO.update

    def counted(self, batch, metrics_out=None):
        run = update(self, batch, metrics_out)
        seen.append(run)
        return run
    monkeypatch.setattr(ESPO, "update", counted)
    model = _run(monkeypatch, f"--environment.nr_envs={N}", f"--algorithm.nr_steps={T}", "--environment.horizon=16",
                 "--algorithm.minibatch_size=512", f"--algorithm.max_epochs={MAX_EPOCHS}", f"--algorithm.total_timesteps={N * T * iters}",
                 "--algorithm.learning_rate=1e-3", "--algorithm.nr_hidden_units=64")
    m = model.last_metrics
    print("espo.hip end to end:", {k: m[k] for k in ("rollout/episode_return", "optim/nr_epochs", "policy/std_dev", "steps/nr_updates")},
          "epochs per iteration", seen)
    assert m["steps/nr_env_steps"] == N * T * iters and len(seen) == iters
    assert m["steps/nr_updates"] == sum(seen) == model.opt_count
    assert all(1 <= r <= MAX_EPOCHS for r in seen) and m["optim/nr_epochs"] == seen[-1]
    for k, v in m.items():
        assert np.isfinite(v), k
    from espo_twin import METRICS
    assert all(k in m for k in METRICS + ("lr/learning_rate", "v_value/explained_variance", "policy/std_dev", "optim/nr_epochs"))
    # reward = -mean_j (clip(a_j) - tanh(obs_j))^2 + noise: a random policy (std 1) scores about -17 per 16-step episode; the bar of
    # test_gpu_train.py::test_runner_train_learns for this task
    assert m["rollout/episode_return"] > -12.0, m["rollout/episode_return"]
    assert m["time/sps"] > 0


def _plugin(tmp_path, alg_over, pidx=None, cidx=None):
    from rlx_amd.runner.config_dict import ConfigDict
    from rlx_amd.runner.default_config import get_config as runner_cfg
    import rlx_amd.algorithms.espo.hip  # noqa: F401
    import rlx_amd.environments.synthetic.random_obs  # noqa: F401
    from rlx_amd.algorithms.algorithm_manager import get_algorithm_config, get_algorithm_model_class
    from rlx_amd.environments.environment_manager import get_environment_config, get_environment_create_train_and_eval_env
    config = ConfigDict()
    config.runner = runner_cfg("train")
    config.runner.save_model = True
    config.algorithm = get_algorithm_config("espo.hip")
    config.environment = get_environment_config("synthetic.random_obs")
    for k, v in dict(nr_envs=32, obs_dim=11, act_dim=3, horizon=8).items():
        config.environment[k] = v
    for k, v in alg_over.items():
        config.algorithm[k] = v
    env, eval_env = get_environment_create_train_and_eval_env("synthetic.random_obs")(config)
    if pidx is not None:
        env.policy_observation_indices, env.critic_observation_indices = pidx, cidx
    return get_algorithm_model_class("espo.hip"), config, env, eval_env


@pytest.mark.parametrize("indices", [False, True])
def test_checkpoint_continues(tmp_path, indices):
    """save / load: parameters, moments, both counters, the acting key and the host generator's state; the loaded model's next
    update draws the rows the saved one would have drawn.  With observation index sets the update reads the full rows."""
    pidx, cidx = (np.arange(0, 6), np.arange(3, 11)) if indices else (None, None)
    over = dict(nr_steps=8, minibatch_size=32, max_epochs=5, total_timesteps=32 * 8 * 3, nr_hidden_units=64, learning_rate=1e-3,
                anneal_learning_rate=True, evaluation_frequency=32 * 8 * 3, evaluation_episodes=4, max_ratio_delta=0.05)
    cls, config, env, eval_env = _plugin(tmp_path, over, pidx, cidx)
    m = cls(config, env, eval_env, str(tmp_path), None)
    assert (m.pdesc.in_dim, m.cdesc.in_dim) == ((6, 8) if indices else (11, 11))
    p0 = m.pparams.clone()
    m.train()
    met = m.last_metrics
    assert 1 <= met["optim/nr_epochs"] <= 5 and met["steps/nr_updates"] == m.opt_count and m.nr_iterations == 3
    assert met["lr/learning_rate"] == pytest.approx(1e-3 * (1 - 3 / 3)) and "eval/episode_return" in met
    assert (m.pparams - p0).abs().max().item() > 0
    m.save()
    config.runner.load_model = os.path.join(str(tmp_path), "models", "best.model")
    m2 = cls.load(config, env, eval_env, str(tmp_path), None, [])
    for k in ("pparams", "pm", "pv", "cparams", "cm", "cv"):
        assert torch.equal(getattr(m2, k), getattr(m, k)), k
    assert (m2.opt_count, m2.nr_iterations) == (m.opt_count, m.nr_iterations) and np.array_equal(m2.key, m.key)
    assert m2.rng.bit_generator.state == m.rng.bit_generator.state
    # the host stream after an early stop is the reference's: `run` lazy draws from the state in front of the update
    B, mb = m.batch_size, m.minibatch_size
    before = m2.rng.bit_generator.state
    lazy = np.random.default_rng(0)
    lazy.bit_generator.state = before
    batch = m2._alloc_batch()
    state, _ = env.reset()
    state, run = m2.train_iteration(batch, state.contiguous())
    first = m2._idx_host.numpy()[0].copy()
    assert np.array_equal(first, lazy.choice(B, size=mb, replace=False))
    for _ in range(run - 1):
        lazy.choice(B, size=mb, replace=False)
    assert m2.rng.bit_generator.state == lazy.bit_generator.state and m2.opt_count == m.opt_count + run
    assert len(m2.test(2)) <= 2
