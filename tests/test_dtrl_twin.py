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



def test_critic_states_equal_to_states_change_no_bit():
    """cstates = states is the shared-observation twin, bit for bit; and the defaults of case() draw what they drew before it had
    options (the numbers the 60 GPU cases were measured on)"""
    c = tw.case(117, 17, 11, 1, 1, 0)
    assert c["cstates"] is None
    base, same = tw.run_case(c), tw.run_case(dict(c, cstates=c["states"].copy()))
    assert base[0] == same[0]
    for a, b in zip(base[1:4], same[1:4]):
        assert np.array_equal(a, b)
    rng = np.random.default_rng(117)
    pp = rng.normal(0, 0.12, c["pspec"].n_params)
    assert np.array_equal(np.asarray(pp[:c["pspec"].logstd], np.float32).astype(np.float64), c["pp"][:c["pspec"].logstd])


def test_permuted_critic_columns_with_permuted_weight_rows_change_nothing():
    """the critic reads cstates and nothing else does: permuting its observation columns together with the rows of its first-layer
    weight leaves the loss and the policy gradient where they were (1e-12), and moves the critic's gradient rows with them"""
    c = tw.case(31, 3, 9, 1, 1, 0, obs=5, cobs=11, chidden=(128, 64))
    assert c["cspec"].in_dim == 11 and c["pspec"].in_dim == 5 and c["cstates"].shape == (9, 11)
    perm = np.random.default_rng(0).permutation(11)
    W = c["cspec"].layers[0]
    n_w = 11 * W["out"]
    cp2 = c["cp"].copy()
    cp2[W["W"]:W["W"] + n_w] = c["cp"][W["W"]:W["W"] + n_w].reshape(11, -1)[perm].reshape(-1)
    base, moved = tw.run_case(c), tw.run_case(dict(c, cp=cp2, cstates=c["cstates"][:, perm]))
    assert abs(base[0] - moved[0]) < 1e-12 and np.abs(base[1] - moved[1]).max() < 1e-12
    assert np.abs(base[2] - moved[2]).max() < 1e-12 and np.abs(base[2]).max() > 1e-4
    g0 = base[3].copy()
    g0[W["W"]:W["W"] + n_w] = base[3][W["W"]:W["W"] + n_w].reshape(11, -1)[perm].reshape(-1)
    assert np.abs(g0 - moved[3]).max() < 1e-12 and np.abs(base[3][W["W"]:W["W"] + n_w]).max() > 1e-6
    # and the critic does not read the policy's observations any more
    other = tw.run_case(dict(c, cstates=c["cstates"] + 1.0))
    assert np.abs(other[3] - base[3]).max() > 1e-6 and np.array_equal(other[2], base[2])
