"""CPU: known answers of tests/dtrl_twin.py, the float64 restatement of PPO-DTRL's loss that the GPU tests compare dtrl.hip with."""
import numpy as np
import pytest

import dtrl_twin as tw
from oracle import ppo

MODES = {"none": (0, 0, 0), "mean": (1, 0, 0), "cov": (0, 1, 0), "entropy": (0, 0, 1), "all": (1, 1, 1)}
I = {k: i for i, k in enumerate(tw.METRICS)}


@pytest.mark.parametrize("A", [1, 3, 8, 17])
@pytest.mark.parametrize("mode", list(MODES))
def test_projections_meet_their_bounds_or_are_the_identity(mode, A):
    """active: KL_mean == mean_bound on every row and KL_cov == cov_bound to 1e-10; inside the bounds both are the identity.  The
    margins the GPU tests need hold at every seed they use (rows included: the three minibatch sizes of test_gpu_dtrl.py)"""
    mean_on, cov_on, ent_on = MODES[mode]
    W = 1 << (A - 1).bit_length()
    for mb in (2, 64 // W + 1, 4 * (64 // W) + 3):
        c = tw.case(100 + A, A, mb, mean_on, cov_on, ent_on)
        _, met, _, _, info = tw.run_case(c)
        assert tw.margins_ok(c, info) and info["cov_on"] == bool(cov_on) and info["ent_on"] == bool(ent_on)
        h = c["h"]
        if mean_on:
            assert abs(met[I["projection/projected_kl_mean"]] - h["mean_bound"]) < 1e-10 and met[I["projection/eta_mu"]] > 0
        else:
            assert met[I["projection/projected_kl_mean"]] == met[I["projection/unprojected_kl_mean"]] and met[I["projection/eta_mu"]] == 0
        if cov_on:
            assert abs(met[I["projection/projected_kl_cov"]] - h["cov_bound"]) < 1e-10 and met[I["projection/eta_cov"]] > 0
        else:
            assert met[I["projection/projected_kl_cov"]] == met[I["projection/unprojected_kl_cov"]] and met[I["projection/eta_cov"]] == 0
        assert np.all(np.isfinite(met))


def test_without_projections_the_twin_is_ppo():
    """all three projections inactive and trust_region_coef = 0: loss, metrics and gradients of oracle/ppo.py"""
    c = tw.case(5, 3, 33, 0, 0, 0)
    c["h"]["trust_region_coef"] = 0.0
    h = c["h"]
    loss, met, gp, gc, info = tw.run_case(c)
    assert not info["cov_on"] and not info["ent_on"] and np.all(info["maha"] < h["mean_bound"])
    l0, m0, gp0, gc0 = ppo.ppo_loss_and_grads(c["pspec"], c["pp"], c["cspec"], c["cp"], c["states"], c["actions"], c["logp_old"], c["returns"],
                                              ppo.normalize_advantages(c["adv"]), h["clip_range"], h["entropy_coef"], h["critic_coef"])
    assert abs(loss - l0) < 1e-12
    for k in ("loss/policy_gradient_loss", "loss/critic_loss", "loss/entropy_loss", "policy_ratio/approx_kl", "policy_ratio/clip_fraction"):
        assert abs(met[I[k]] - m0[k]) < 1e-12, k
    assert np.abs(gp - gp0).max() < 1e-12 and np.abs(gc - gc0).max() < 1e-12 and np.abs(gp0).max() > 1e-4

