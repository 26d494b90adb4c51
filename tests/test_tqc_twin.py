"""CPU: the TQC twin (tests/tqc_twin.py) -- hand-computed answers of the pair loss, the pooled truncation, the three gradients
against float64 torch.autograd -- and the registration of the `tqc.hip` plugin with the reference's defaults."""
import types

import numpy as np
import pytest

import tqc_twin as tw
from oracle import sac

H0 = dict(gamma=0.99, target_entropy=-2.0, ensemble_size=1, nr_atoms_per_net=1, nr_dropped_atoms_per_net=0, huber_kappa=1.0)


def _loss(q, y, kappa):
    loss, dq = tw.pair_loss(np.asarray(q, np.float64), np.asarray(y, np.float64), kappa)
    return loss, dq


# ------------------------------------------------------------------------------------------------- the pair loss, by hand
def test_pair_loss_linear_branch():
    """T = K = 1, q = 0, y = 2, kappa = 1: delta = 2 > kappa -> huber = 1 (2 - 0.5) = 1.5, w = |0.5 - 0| = 0.5 -> 0.75;
    d/dq = -w clamp(delta) / kappa = -0.5"""
    loss, dq = _loss([[0.0]], [[2.0]], 1.0)
    assert loss[0] == pytest.approx(0.75, abs=1e-15) and dq[0, 0] == pytest.approx(-0.5, abs=1e-15)


def test_pair_loss_quadratic_branch_negative_delta():
    """q = 0, y = -0.5: huber = 0.125, w = |0.5 - 1| = 0.5 -> 0.0625; d/dq = -0.5 * (-0.5) = +0.25"""
    loss, dq = _loss([[0.0]], [[-0.5]], 1.0)
    assert loss[0] == pytest.approx(0.0625, abs=1e-15) and dq[0, 0] == pytest.approx(0.25, abs=1e-15)


def test_pair_loss_two_quantile_levels():
    """T = 2, K = 1, q = (0, 0), y = 0.5: tau = (0.25, 0.75), delta = 0.5 for both, huber = 0.125 ->
    loss = (0.25 + 0.75) 0.125 / 2 = 0.0625; d/dq_i = -tau_i 0.5 / 2"""
    loss, dq = _loss([[0.0, 0.0]], [[0.5]], 1.0)
    assert loss[0] == pytest.approx(0.0625, abs=1e-15)
    np.testing.assert_allclose(dq[0], [-0.0625, -0.1875], atol=1e-15)
    # negative delta: the weights swap to 1 - tau
    loss, dq = _loss([[0.0, 0.0]], [[-0.5]], 1.0)
    np.testing.assert_allclose(dq[0], [0.1875, 0.0625], atol=1e-15)


def test_pair_loss_kappa_two():
    """kappa = 2 exercises the / kappa: q = 0, y = 1 -> quadratic, 0.5 * 0.5 / 2 = 0.125, d/dq = -0.5 * 1 / 2 = -0.25;
    y = 5 -> linear, 0.5 * 2 (5 - 1) / 2 = 2.0, d/dq = -0.5 * 2 / 2 = -0.5"""
    loss, dq = _loss([[0.0]], [[1.0]], 2.0)
    assert loss[0] == pytest.approx(0.125, abs=1e-15) and dq[0, 0] == pytest.approx(-0.25, abs=1e-15)
    loss, dq = _loss([[0.0]], [[5.0]], 2.0)
    assert loss[0] == pytest.approx(2.0, abs=1e-15) and dq[0, 0] == pytest.approx(-0.5, abs=1e-15)


def test_pair_loss_huge_kappa_is_a_quarter_of_the_squared_differences():
    """E = 2, N = 1, dropped = 0 (T = K = 2), kappa huge: every pair is on the quadratic branch, so the pair broadcast is all that
    is left: loss kappa = 1/4 sum_{i,k} w_ik (y_k - q_i)^2 / 2, w_ik = |tau_i - [y_k < q_i]|, tau = (0.25, 0.75) -- the mean over
    the four pairs.  With equal atoms q = (a, a) the weights of a column add to tau_0 + tau_1 = 1 (or 2 - 1) for either sign and
    the sum over the pairs loses them: loss kappa T K = sum_k (y_k - a)^2 / 2 = 1/4 sum_{i,k} (y_k - q_i)^2."""
    rng = np.random.default_rng(0)
    kappa = 1e6
    tau = np.array([0.25, 0.75])
    for _ in range(5):
        q, y = rng.standard_normal((1, 2)), rng.standard_normal((1, 2))
        delta = y[:, None, :] - q[:, :, None]                              # [1, i, k]
        loss, _ = _loss(q, y, kappa)
        assert loss[0] * kappa == pytest.approx(0.25 * (np.abs(tau[None, :, None] - (delta < 0)) * 0.5 * delta ** 2).sum(), rel=1e-12)
        q = np.repeat(rng.standard_normal((1, 1)), 2, axis=1)
        loss, _ = _loss(q, y, kappa)
        assert loss[0] * kappa * 4 == pytest.approx(0.25 * ((y[:, None, :] - q[:, :, None]) ** 2).sum(), rel=1e-12)


def test_truncation_takes_the_smallest_of_the_pooled_atoms():
    """two nets with disjoint ranges (net 0 in [0, 1), net 1 in [10, 11)), N = 4, dropped = 2 per net: K = 4 of the POOLED eight
    = all of net 0 and none of net 1 -- every dropped atom comes from one net (per-net truncation would keep two of each)"""
    rng = np.random.default_rng(1)
    z0, z1 = rng.random((3, 4)), 10.0 + rng.random((3, 4))
    atoms = np.concatenate([z0, z1], axis=1)
    r, term, nlogp = rng.standard_normal(3), np.array([0.0, 1.0, 0.0]), rng.standard_normal(3)
    y = tw.truncated_target(atoms, r, term, 0.7, nlogp, 0.99, 4)
    exp = r[:, None] + 0.99 * (1 - term)[:, None] * (np.sort(z0, axis=1) - 0.7 * nlogp[:, None])
    np.testing.assert_allclose(y, exp, rtol=0, atol=1e-15)
    assert np.all(np.diff(y[[0, 2]], axis=1) >= 0) and np.all(y[1] == r[1])


# ------------------------------------------------------------------------------------------- the twin against torch.autograd
def _problem(seed, Op, Oc, A, ph, qh, E, N, dropped, B, kappa=1.0):
    rng = np.random.default_rng(seed)
    ps, qs = tw.make_specs(Op, Oc, A, ph, qh, N)
    pp = sac.lecun_normal_init(ps, rng, np.float64) + 0.02 * rng.standard_normal(ps.n_params)
    pp[ps.head["W"]:ps.head["W"] + ps.head["in"] * ps.head["out"]] *= 0.1
    qp = np.concatenate([sac.lecun_normal_init(qs, rng, np.float64) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params)
    qtp = qp + 0.01 * rng.standard_normal(qp.shape)
    asym = Op != Oc
    batch = dict(states=rng.standard_normal((B, Op)), next_states=rng.standard_normal((B, Op)), actions=np.tanh(rng.standard_normal((B, A))),
                 rewards=rng.standard_normal(B), terminations=(rng.random(B) < 0.2).astype(np.float64))
    extra = dict(critic_states=rng.standard_normal((B, Oc)), critic_next_states=rng.standard_normal((B, Oc))) if asym else {}
    h = dict(H0, ensemble_size=E, nr_atoms_per_net=N, nr_dropped_atoms_per_net=dropped, huber_kappa=kappa, target_entropy=-float(A))
    eps = rng.standard_normal((2, B, A))
    return ps, qs, pp, qp, qtp, batch, extra, h, eps


@pytest.mark.parametrize("Op,Oc,A,ph,qh,E,N,dropped,B,kappa", [
    (5, 5, 2, [16, 16], [16, 16], 2, 5, 1, 7, 1.0),
    (6, 4, 3, [8], [12, 8, 8], 3, 4, 0, 5, 0.3),        # own critic columns, one and three hidden layers, both Huber branches
    (4, 4, 1, [8, 8], [8, 8], 1, 9, 3, 6, 2.5),
])
def test_twin_gradients_match_torch_autograd(Op, Oc, A, ph, qh, E, N, dropped, B, kappa):
    ps, qs, pp, qp, qtp, b, extra, h, eps = _problem(Op + B, Op, Oc, A, ph, qh, E, N, dropped, B, kappa)
    la = np.float64(-0.3)
    args = (ps, pp, qs, qp, qtp, la, b["states"], b["next_states"], b["actions"], b["rewards"], b["terminations"], eps[0], eps[1], h)
    met, gp, gq, ga, aux = tw.loss_and_grads(*args, **extra)
    loss_t, gp_t, gq_t, ga_t = tw.loss_torch(*args, **extra)
    assert met["loss/q_loss"] + met["loss/policy_loss"] + met["loss/entropy_loss"] == pytest.approx(loss_t, rel=1e-12)
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    assert rel(gp, gp_t) < 1e-10 and rel(gq, gq_t) < 1e-10 and abs(ga - ga_t) <= 1e-10 * abs(ga_t)
    assert np.linalg.norm(gq_t) > 0 and np.linalg.norm(gp_t) > 0
    # both Huber branches are in play where kappa is small
    d = np.abs(aux["y"][:, None, :] - aux["q_atoms"][:, :, None])
    if kappa < 1.0:
        assert (d > kappa).any() and (d <= kappa).any()


def test_twin_update_applies_adam_and_polyak():
    ps, qs, pp, qp, qtp, b, extra, h, eps = _problem(3, 5, 5, 2, [8, 8], [8, 8], 2, 3, 1, 6)
    st = tw.zero_state(pp, qp, qtp, -0.3)
    batch = (b["states"], b["next_states"], b["actions"], b["rewards"], b["terminations"])
    new, met, (gp, gq, ga), aux = tw.update(ps, qs, st, batch, eps[0], eps[1], h, 3e-4, 0.005)
    assert new["count"] == 1
    np.testing.assert_allclose(new["pm"], 0.1 * gp, rtol=1e-12)
    np.testing.assert_allclose(new["qv"], 0.001 * gq * gq, rtol=1e-9)
    big = np.abs(gq) > 1e-4                                    # eps / |g| = 1e-8 / 1e-4 is inside the tolerance
    np.testing.assert_allclose((new["Q"] - st["Q"])[big], -3e-4 * np.sign(gq[big]), rtol=1e-3)       # first Adam step
    np.testing.assert_allclose(new["QT"], 0.005 * new["Q"] + 0.995 * st["QT"], rtol=1e-14)
    assert met["gradients/critic_grad_norm"] == pytest.approx(np.linalg.norm(gq))
    new2, _, _, _ = tw.update(ps, qs, new, batch, eps[1], eps[0], h, 3e-4, 0.005)
    assert new2["count"] == 2 and not np.array_equal(new2["am"], new["am"])
    # a ReLU inverted in the reverse pass for one sample of critic 1: that critic's gradient moves by critic_kink_delta, nothing else does
    args = (ps, st["P"], qs, st["Q"], st["QT"], st["la"][0], *batch, eps[0], eps[1], h)
    _, gp_k, gq_k, _, _ = tw.loss_and_grads(*args, relu_toggle=[("q1", 1, 4, 3)])
    n = qs.n_params
    x = np.concatenate([batch[0], batch[2]], axis=1)
    delta = tw.critic_kink_delta(qs, st["Q"][n:], x[4:5], aux["dq"][4:5, 3:], 1, 3)
    assert np.array_equal(gp_k, gp) and np.array_equal(gq_k[:n], gq[:n]) and np.linalg.norm(delta) > 0
    np.testing.assert_allclose(gq_k[n:] - gq[n:], delta, rtol=1e-9, atol=1e-18)


# ---------------------------------------------------------------------------------------------------------- the plugin
REFERENCE_DEFAULTS = dict(                                   # rl_x/algorithms/tqc/flax/default_config.py:9-28
    device="gpu", total_timesteps=1e9, learning_rate=3e-4, anneal_learning_rate=False, buffer_size=1e6, learning_starts=5000,
    batch_size=256, tau=0.005, gamma=0.99, ensemble_size=2, nr_atoms_per_net=25, nr_dropped_atoms_per_net=2, huber_kappa=1.0,
    target_entropy="auto", log_std_min=-20, log_std_max=2, nr_hidden_units=256, logging_frequency=3000, evaluation_frequency=-1,
    evaluation_episodes=10)


def test_tqc_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    from rlx_amd.runner.runner import Runner
    assert Runner._import_plugin("algorithms", "tqc.hip", ["rlx_amd"]) == "rlx_amd"
    import rlx_amd.algorithms.tqc.hip as plugin
    assert plugin.TQC_HIP == "tqc.hip"
    cfg = am.get_algorithm_config("tqc.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("tqc.hip")
    assert model.__name__ == "TQC"
    from rlx_amd.algorithms.sac.hip.sac import SAC
    assert issubclass(model, SAC)
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


@pytest.mark.parametrize("flags, msg", [
    (dict(device="cpu"), "MI355X"), (dict(ensemble_size=9), "ensemble_size"), (dict(ensemble_size=0), "ensemble_size"),
    (dict(ensemble_size=6, nr_atoms_per_net=25), "at most 128"), (dict(nr_dropped_atoms_per_net=25), "nr_dropped_atoms_per_net"),
    (dict(huber_kappa=0.0), "huber_kappa")])
def test_tqc_hip_refuses_what_it_cannot_run(flags, msg):
    """raised in front of anything that touches a device"""
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.tqc.hip  # noqa: F401
    cfg = am.get_algorithm_config("tqc.hip")
    for k, v in flags.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    config = sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
                environment=sn(seed=0, nr_envs=8))
    with pytest.raises(ValueError, match=msg):
        am.get_algorithm_model_class("tqc.hip")(config, None, None, "/nonexistent", None)
