"""CPU: the REDQ twin (tests/redq_twin.py) -- hand-computed answers, the gradients against float64 torch.autograd, the dependence
of every step on the one before it -- the host-only target subset of the library against oracle/prng.py, and the registration of
the `redq.hip` plugin with the reference's defaults."""
import types

import numpy as np
import pytest

import redq_twin as tw
from oracle import prng

LR, TAU = 3e-4, 0.005


# ------------------------------------------------------------------------------------------------------------ by hand
def test_critic_loss_by_hand():
    """E = 2, B = 1, M = 2: q = (1, 3), targets (0.5, 2), r = 1, gamma = 0.5, alpha = 2, logp' = 0.25:
    y = 1 + 0.5 (0.5 - 0.5) = 1; loss = ((1 - 1)^2 + (3 - 1)^2) / 2 = 2; dq = 2 (q - y) / (B E) = (0, 2)"""
    y, loss, dq = tw.critic_loss(np.array([[1.0, 3.0]]), np.array([[0.5, 2.0]]), np.array([1.0]), np.array([0.0]), 2.0, np.array([0.25]), 0.5)
    assert y[0] == 1.0 and loss[0] == 2.0 and np.array_equal(dq, [[0.0, 2.0]])
    # terminated: y = r whatever the targets say
    y, _, _ = tw.critic_loss(np.array([[1.0, 3.0]]), np.array([[7.0, -9.0]]), np.array([0.3]), np.array([1.0]), 2.0, np.array([0.25]), 0.5)
    assert y[0] == 0.3
    # M = 1: the one selected target, not the smaller of the ensemble
    y, _, _ = tw.critic_loss(np.array([[1.0, 3.0]]), np.array([[2.0]]), np.array([0.0]), np.array([0.0]), 0.0, np.array([0.0]), 1.0)
    assert y[0] == 2.0


def test_policy_seed_by_hand():
    """E = 2, B = 1: the gradient of -min goes to the smaller critic; an exact tie splits it evenly.  E = 3, B = 2: per-row minima"""
    mn, seed = tw.policy_seed(np.array([[1.0, 3.0]]))
    assert mn[0] == 1.0 and np.array_equal(seed, [[-1.0, 0.0]])
    mn, seed = tw.policy_seed(np.array([[2.0, 2.0]]))
    assert mn[0] == 2.0 and np.array_equal(seed, [[-0.5, -0.5]])
    mn, seed = tw.policy_seed(np.array([[5.0, 4.0, 6.0], [1.0, 7.0, 1.0]]))
    assert np.array_equal(mn, [4.0, 1.0]) and np.array_equal(seed, [[0.0, -0.5, 0.0], [-0.25, 0.0, -0.25]])


# ------------------------------------------------------------------------------------------- the twin against torch.autograd
def _case(seed=3, **kw):
    args = dict(O=5, A=2, B=7, ph=[64], qh=[64], E=3, M=2, G=2)
    args.update(kw)
    p = tw.problem(seed, **args)
    rng = np.random.default_rng(seed + 1)
    G, B, A, E, M = args["G"], args["B"], args["A"], args["E"], args["M"]
    p["eps1"], p["eps2"] = rng.standard_normal((G, B, A)), rng.standard_normal((B, A))
    p["subsets"] = np.array([rng.permutation(E)[:M] for _ in range(G)])
    return p


def _update(p, st=None, lr_critic=LR, delta=0.0):
    cb = p["cbatch"] or (None, None)
    return tw.update(p["ps"], p["qs"], p["state"] if st is None else st, p["batch"], p["eps1"], p["eps2"], p["subsets"], p["h"], LR, lr_critic,
                     delta, LR, TAU, cb[0], cb[1])


@pytest.mark.parametrize("Oc", [None, 4])
def test_twin_gradients_match_torch_autograd(Oc):
    """O 5, A 2, B 7, E 3, M 2, G 2, hidden [64]: step 0's critic gradient and -- with the critics left as they are (critic learning
    rate 0, so Adam and Polyak move nothing the policy step reads) -- the policy's and alpha's, at 1e-10"""
    p = _case(Oc=Oc)
    st = p["state"]
    new, met, g, ys = _update(p, lr_critic=0.0)
    assert np.array_equal(new["Q"], st["Q"])
    cb = p["cbatch"] or (None, None)
    b0 = tuple(x[0] for x in p["batch"])
    ql, gQ, pel, gP, gLA = tw.losses_torch(p["ps"], st["P"], p["qs"], st["Q"], st["QT"], st["la"][0], b0, p["eps1"][0], p["eps2"], p["subsets"][0],
                                           p["h"], None if cb[0] is None else cb[0][0], None if cb[1] is None else cb[1][0])
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    assert rel(g["gq"][0], gQ) < 1e-10 and rel(g["gp"], gP) < 1e-10 and abs(g["ga"] - gLA) <= 1e-10 * abs(gLA)
    assert np.linalg.norm(gQ) > 0 and np.linalg.norm(gP) > 0
    assert met["loss/policy_loss"] + met["loss/entropy_loss"] == pytest.approx(pel, rel=1e-12)
    # no ties in this case: every row's seed went to one critic
    assert met["gradients/policy_grad_norm"] == pytest.approx(np.linalg.norm(gP), rel=1e-10)


def test_twin_update_counters_means_adam_and_polyak():
    p = _case(G=3)
    st = p["state"]
    new, met, g, ys = _update(p, delta=-1e-5)
    assert (new["q_count"], new["pi_count"]) == (3, 1) and ys.shape == (3, 7)
    assert met["gradients/critic_grad_norm"] == pytest.approx(np.mean([np.linalg.norm(x) for x in g["gq"]]), rel=1e-14)
    np.testing.assert_allclose(new["pm"], 0.1 * g["gp"], rtol=1e-12)
    # the critics' first moment after three steps from zero: 0.1 (0.81 g0 + 0.9 g1 + g2)
    np.testing.assert_allclose(new["qm"], 0.1 * (0.81 * g["gq"][0] + 0.9 * g["gq"][1] + g["gq"][2]), rtol=1e-9, atol=1e-18)
    # one step alone: Adam's first step is -lr sign(g), and Polyak follows it
    p1 = _case(G=1)
    n1, _, g1, _ = _update(p1)
    big = np.abs(g1["gq"][0]) > 1e-4
    np.testing.assert_allclose((n1["Q"] - p1["state"]["Q"])[big], -LR * np.sign(g1["gq"][0][big]), rtol=1e-3)
    np.testing.assert_allclose(n1["QT"], TAU * n1["Q"] + (1 - TAU) * p1["state"]["QT"], rtol=1e-14)
    assert not np.array_equal(n1["la"], p1["state"]["la"]) and not np.array_equal(new["P"], st["P"])


def test_every_step_sees_the_one_before():
    """step 2's y comes from the targets step 1's Polyak left and its gradient from the critics step 1's Adam left: with step 1's
    learning rate zeroed (lr_critic 0, delta = LR: steps run at 0, LR) step 2's y and gradient change, step 1's do not; and the
    policy step reads the critics from after step G: zeroing every critic step changes its gradient"""
    p = _case(G=2)
    new, met, g, ys = _update(p)
    new0, met0, g0, ys0 = _update(p, lr_critic=0.0, delta=LR)
    assert np.array_equal(ys0[0], ys[0]) and np.array_equal(g0["gq"][0], g["gq"][0])
    assert np.abs(ys0[1] - ys[1]).max() > 1e-9 and np.linalg.norm(g0["gq"][1] - g["gq"][1]) > 1e-9 * np.linalg.norm(g["gq"][1])
    # by hand: at learning rate 0 step 1 leaves the critics alone and its Polyak step still moves the targets towards them; step 2
    # of the zeroed run equals a single step on batch 1 from that state
    st = p["state"]
    one = dict(p, batch=tuple(x[1:] for x in p["batch"]), eps1=p["eps1"][1:], subsets=p["subsets"][1:], h=dict(p["h"], q_update_steps=1),
               state=dict(st, QT=TAU * st["Q"] + (1 - TAU) * st["QT"]))
    _, _, g_one, ys_one = _update(one)
    assert np.array_equal(ys_one[0], ys0[1]) and np.array_equal(g_one["gq"][0], g0["gq"][1])
    _, metz, gz, _ = _update(p, lr_critic=0.0, delta=0.0)
    assert np.linalg.norm(gz["gp"] - g["gp"]) > 1e-9 * np.linalg.norm(g["gp"])
    assert metz["q_value/q_value"] != met["q_value/q_value"]


# ------------------------------------------------------------------------------------------------- the library's host-only part
@pytest.mark.parametrize("scheme", [1, 0])
def test_subset_host_equals_the_oracle_permutation(scheme):
    """rlx_redq_subset_host = permutation(sample_key, E)[:M] for every E in 1..16, M in {1, E}, 8 keys each; E = 1 gives [0]"""
    from rlx_amd.hip import redq_subset
    for E in range(1, 17):
        for k in range(8):
            key = prng.split(prng.prng_key(1000 * E + k), 3, bool(scheme))[2]
            exp = prng.permutation_rows(key, np.arange(E)[None], bool(scheme))[0]
            assert sorted(exp) == list(range(E))
            for M in {1, E}:
                got = redq_subset(key, E, M, scheme)
                assert got.dtype == np.int32 and np.array_equal(got, exp[:M]), (E, M, k, got, exp)
    assert np.array_equal(redq_subset(prng.prng_key(5), 1, 1, scheme), [0])


def test_subset_host_refuses_bad_sizes():
    from rlx_amd.hip import RlxError, redq_subset
    for E, M in ((0, 1), (17, 1), (3, 0), (3, 4)):
        with pytest.raises(RlxError, match="rc=-1"):
            redq_subset(prng.prng_key(1), E, M)


# ---------------------------------------------------------------------------------------------------------- the plugin
REFERENCE_DEFAULTS = dict(                                   # rl_x/algorithms/redq/flax/default_config.py:9-27
    device="gpu", total_timesteps=1e9, learning_rate=3e-4, anneal_learning_rate=False, buffer_size=1e6, learning_starts=5000,
    batch_size=256, tau=0.005, gamma=0.99, ensemble_size=10, in_target_minimization_size=2, q_update_steps=20,
    target_entropy="auto", log_std_min=-20, log_std_max=2, nr_hidden_units=256, logging_frequency=100, evaluation_frequency=-1,
    evaluation_episodes=10)


def test_redq_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    from rlx_amd.runner.runner import Runner
    assert Runner._import_plugin("algorithms", "redq.hip", ["rlx_amd"]) == "rlx_amd"
    import rlx_amd.algorithms.redq.hip as plugin
    assert plugin.REDQ_HIP == "redq.hip"
    cfg = am.get_algorithm_config("redq.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("redq.hip")
    assert model.__name__ == "REDQ"
    from rlx_amd.algorithms.sac.hip.sac import SAC
    assert issubclass(model, SAC)
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


@pytest.mark.parametrize("flags, msg", [
    (dict(device="cpu"), "MI355X"), (dict(ensemble_size=17), "ensemble_size"), (dict(ensemble_size=0), "ensemble_size"),
    (dict(in_target_minimization_size=11), "in_target_minimization_size"), (dict(in_target_minimization_size=0), "in_target_minimization_size"),
    (dict(q_update_steps=0), "q_update_steps"), (dict(q_update_steps=65), "q_update_steps"),
    (dict(network_architecture="full_jit"), "flax networks"), (dict(enable_observation_normalization=True), "observation normalisation")])
def test_redq_hip_refuses_what_it_cannot_run(flags, msg):
    """raised in front of anything that touches a device"""
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.redq.hip  # noqa: F401
    cfg = am.get_algorithm_config("redq.hip")
    for k, v in flags.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    config = sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
                environment=sn(seed=0, nr_envs=8))
    with pytest.raises(ValueError, match=msg):
        am.get_algorithm_model_class("redq.hip")(config, None, None, "/nonexistent", None)


def test_redq_hip_schedules():
    """redq.py:82-98: the critics' schedule divides by q_update_steps and counts critic steps; inside one call it moves by a
    constant per step"""
    from rlx_amd.algorithms.redq.hip.redq import critic_lr_and_delta, policy_lr
    kw = dict(learning_rate=3e-4, nr_envs=4, learning_starts=100, total_timesteps=10100, q_update_steps=5)
    ref_q = lambda count: 3e-4 * (1.0 - ((count * 4) - 100) / ((10100 - 100) * 5))
    ref_p = lambda count: 3e-4 * (1.0 - ((count * 4) - 100) / (10100 - 100))
    lr, delta = critic_lr_and_delta(35, anneal=True, **kw)
    assert lr == pytest.approx(ref_q(35), rel=1e-14) and lr + 3 * delta == pytest.approx(ref_q(38), rel=1e-12)
    assert policy_lr(7, anneal=True, **kw) == pytest.approx(ref_p(7), rel=1e-14)
    assert critic_lr_and_delta(35, anneal=False, **kw) == (3e-4, 0.0) and policy_lr(7, anneal=False, **kw) == 3e-4
