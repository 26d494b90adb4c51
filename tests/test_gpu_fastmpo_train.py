"""GPU: the `fastmpo.hip` plugin end to end on synthetic.random_obs for a few hundred env steps: the fill phase, acting with the target
policy, the n-step ring, ONE sample and ONE normaliser merge per iteration, rlx_fastmpo_update_f32, the 28 metrics, evaluation and a
save / load round trip.  Metrics finite; the target networks and log_alpha_mean move."""
import os

import numpy as np
import pytest
import torch

import fastmpo_twin as tw

pytestmark = pytest.mark.gpu


def _plugin(env_over, alg_over, pidx=None, cidx=None):
    from rlx_amd.runner.config_dict import ConfigDict
    from rlx_amd.runner.default_config import get_config as runner_cfg
    import rlx_amd.algorithms.fastmpo.hip  # noqa: F401
    import rlx_amd.environments.synthetic.random_obs  # noqa: F401
    from rlx_amd.algorithms.algorithm_manager import get_algorithm_config, get_algorithm_model_class
    from rlx_amd.environments.environment_manager import get_environment_config, get_environment_create_train_and_eval_env
    config = ConfigDict()
    config.runner = runner_cfg("train")
    config.algorithm = get_algorithm_config("fastmpo.hip")
    config.environment = get_environment_config("synthetic.random_obs")
    for k, v in env_over.items():
        config.environment[k] = v
    for k, v in alg_over.items():
        config.algorithm[k] = v
    env, eval_env = get_environment_create_train_and_eval_env("synthetic.random_obs")(config)
    if pidx is not None:
        env.policy_observation_indices, env.critic_observation_indices = pidx, cidx
    return get_algorithm_model_class("fastmpo.hip"), config, env, eval_env


@pytest.mark.parametrize("variant", ["defaults", "single_clipped_actions", "columns"])
def test_plugin_trains_end_to_end(dev, tmp_path, variant):
    alg = dict(batch_size=32, buffer_size_per_env=8, learning_starts=3, n_steps=1, total_timesteps=16 * 20, logging_frequency=16 * 10,
               evaluation_and_save_frequency=16 * 10, evaluation_active=True, nr_policy_updates_per_step=2, nr_critic_updates_per_policy_update=2)
    pidx = cidx = None
    if variant == "single_clipped_actions":
        alg.update(dual_critic=False, critic_network_type="mpo", policy_network_type="fasttd3", action_clipping=True, action_rescaling="normal",
                   n_steps=3, collect_data_with_online_policy=True)
    if variant == "columns":
        alg.update(clipped_double_q_learning=True, action_rescaling="fastsac", critic_network_type="fasttd3")
        pidx, cidx = np.arange(0, 10), np.arange(4, 20)
    cls, config, env, eval_env = _plugin(dict(nr_envs=16, obs_dim=20, act_dim=3, horizon=10, termination_probability=0.1), alg, pidx, cidx)
    config.runner.save_model = True
    m = cls(config, env, eval_env, str(tmp_path), None)
    steps, real_final = [], m._final_next_state

    def recording_final(next_state, done, info):      # what the env returned at every TRAINING vector step (evaluation steps the env too)
        steps.append((next_state.clone(), done.clone(), info["final_observation"].clone()))
        return real_final(next_state, done, info)
    m._final_next_state = recording_final
    p0, q0, tp0, tq0, d0 = (x.clone() for x in (m.pparams, m.qparams, m.tpparams, m.tqparams, m.duals))
    m.train()
    met = m.last_metrics
    for name in tw.METRICS:
        assert name in met and np.isfinite(met[name]), (name, met)
    assert m.opt_counts == (20 * 4, 20 * 2, 20 * 2) and met["steps/nr_env_steps"] == 16 * 20
    assert m.size == 8 and m.pos == (3 + 20) % 8                 # the ring wrapped: the full-ring sampling path ran
    # the ring's next state of an env whose episode ended is the observation it ended on, not the auto-reset one (fastmpo.py:247)
    ended = 0
    for i in range(len(steps) - 8, len(steps)):
        nxt, done, fin = steps[i]
        row = m.ring[1][i % 8]
        assert torch.equal(row[done], fin[done]) and torch.equal(row[~done], nxt[~done])
        assert not torch.equal(fin[done], nxt[done]) or not bool(done.any())
        ended += int(done.sum())
    assert len(steps) == 23 and ended > 0
    for new, old in ((m.pparams, p0), (m.qparams, q0), (m.tpparams, tp0), (m.tqparams, tq0)):
        assert (new - old).abs().max().item() > 0                # the online and the TARGET networks moved
    assert not torch.equal(m.tpparams, m.pparams) and not torch.equal(m.tqparams, m.qparams)      # Polyak, not a copy
    A = m.act_dim
    assert (m.duals[1:1 + A] - d0[1:1 + A]).abs().min().item() > 0                                  # log_alpha_mean moves
    if m.obs_norm:
        assert int(m.norm_count.item()) == 20 * 2 * 4 * 32      # one merge of 2 P G B rows per iteration
    assert "eval/episode_return" in met
    if variant == "single_clipped_actions":
        assert met["lr/critic_learning_rate"] == pytest.approx(3e-4) and met["dual/penalty_temperature"] > 0
        # the schedules follow each optimiser's own step count (fastmpo.py:126-146): lr (1 - count nr_envs / total_timesteps)
        m.anneal, m.total_timesteps = (True, False, True), 16 * 1000
        c_lr, p_lr, d_lr = m.learning_rates()
        assert np.allclose(c_lr, 3e-4 * (1.0 - (80 + np.arange(4)) * 16 / 16000.0)) and np.allclose(p_lr, [3e-4, 3e-4])
        assert np.allclose(d_lr, 1e-2 * (1.0 - (40 + np.arange(2)) * 16 / 16000.0))
    m.save()
    config.runner.load_model = os.path.join(str(tmp_path), "models", "latest.model")
    m2 = cls.load(config, env, eval_env, str(tmp_path), None, [])
    for k in cls._STATE:
        assert torch.equal(getattr(m2, k), getattr(m, k)), k
    assert m2.opt_counts == m.opt_counts and np.array_equal(m2.key, m.key) and len(m2.test(2)) <= 2
