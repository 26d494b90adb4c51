"""GPU: `ppo_dtrl.hip` end to end through the reference-style entry point (Runner -> registry -> ppo_dtrl.hip on synthetic.random_obs)
with bounds tight enough that the projections fire: every metric is finite and every update's projected KL parts respect their bounds."""
import sys

import numpy as np
import pytest

from test_gpu_dtrl import ETA_TOL

pytestmark = pytest.mark.gpu
MEAN_BOUND, COV_BOUND = 1e-4, 1e-6


def test_runner_train_keeps_the_trust_region(monkeypatch):
    from rlx_amd.algorithms.ppo_dtrl.hip.ppo_dtrl import METRIC_NAMES, PPODTRL
    from rlx_amd.runner.runner import Runner
    iters, N, T, rows = 4, 64, 16, []
    update = PPODTRL.update

    def recorded(self, batch, metrics_out):
        update(self, batch, metrics_out)
        rows.append(metrics_out.cpu().numpy().copy())
    monkeypatch.setattr(PPODTRL, "update", recorded)
    monkeypatch.setattr(sys, "argv", [
        "experiment.py", "--algorithm.name=ppo_dtrl.hip", "--environment.name=synthetic.random_obs", "--runner.mode=train",
        f"--environment.nr_envs={N}", f"--algorithm.nr_steps={T}", "--environment.horizon=8", "--algorithm.minibatch_size=256",
        "--algorithm.nr_epochs=3", f"--algorithm.total_timesteps={N * T * iters}", "--algorithm.learning_rate=3e-3",
        f"--algorithm.mean_bound={MEAN_BOUND}", f"--algorithm.cov_bound={COV_BOUND}", "--algorithm.evaluation_and_save_frequency=-1"])
    model = Runner().run()
    m = model.last_metrics
    assert m["steps/nr_env_steps"] == N * T * iters and m["steps/nr_updates"] == model.opt_count == iters * 3 * 4 == sum(len(r) for r in rows)
    for k, v in m.items():
        assert np.isfinite(v), k
    assert all(k in m for k in METRIC_NAMES + ["lr/learning_rate", "v_value/explained_variance", "policy/std_dev"])
    met = np.concatenate(rows)
    i = METRIC_NAMES.index
    assert np.all(np.isfinite(met))
    assert np.all(met[:, i("projection/projected_kl_mean")] <= MEAN_BOUND * (1 + ETA_TOL))
    assert np.all(met[:, i("projection/projected_kl_cov")] <= COV_BOUND * (1 + ETA_TOL))
    # the projections did fire: both multipliers are positive somewhere, and the unprojected parts exceeded their bounds there
    assert met[:, i("projection/eta_mu")].max() > 0 and met[:, i("projection/eta_cov")].max() > 0
    assert met[:, i("projection/unprojected_kl_mean")].max() > MEAN_BOUND and met[:, i("projection/unprojected_kl_cov")].max() > COV_BOUND
