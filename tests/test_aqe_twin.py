"""CPU: the AQE twin (tests/aqe_twin.py) -- hand-computed answers, the gradients against float64 torch.autograd, the dependence of
every step on the one before it -- and the registration of the `aqe.hip` plugin with the reference's defaults, its schedules and
its refusals."""
import types

import numpy as np
import pytest

import aqe_twin as tw

LR, TAU = 3e-4, 0.005
A1 = lambda *v: np.array(v, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ by hand
def test_truncated_mean_and_critic_loss_by_hand():
    """E 2, H 2, dropped 1, B 1: the pooled targets (3, -1, 2, 0) -> mean of the three lowest (-1, 0, 2) = 1/3; r = 1, gamma = 0.5,
    alpha = 1, logp' = 1/3: y = 1 + 0.5 (1/3 - 1/3) = 1; q = (0, 1, 2, 3): loss = (1 + 0 + 1 + 4) / 4 = 1.5, dq = 2 (q - 1) / 4"""
    qn = np.array([[3.0, -1.0, 2.0, 0.0]])
    assert tw.truncated_mean_target(qn, 3)[0] == pytest.approx(1.0 / 3.0, rel=1e-15)
    y, loss, dq = tw.critic_loss(np.array([[0.0, 1.0, 2.0, 3.0]]), qn, A1(1.0), A1(0.0), 1.0, A1(1.0 / 3.0), 0.5, 3)
    assert y[0] == pytest.approx(1.0, abs=1e-15) and loss[0] == pytest.approx(1.5, rel=1e-14)
    np.testing.assert_allclose(dq, [[-0.5, 0.0, 0.5, 1.0]], atol=1e-15)
    # terminated: y = r whatever the targets say
    y, _, _ = tw.critic_loss(np.array([[0.0, 1.0, 2.0, 3.0]]), np.array([[7.0, -9.0, 1e3, 4.0]]), A1(0.3), A1(1.0), 1.0, A1(0.25), 0.5, 3)
    assert y[0] == 0.3


def test_truncated_mean_edges_by_hand():
    qn = np.array([[3.0, -1.0, 2.0, 0.0], [5.0, 5.0, 1.0, 9.0]])
    # dropped = 0: the plain mean over the pool
    np.testing.assert_allclose(tw.truncated_mean_target(qn, 4), [1.0, 5.0], rtol=1e-15)
    # K = 1: the pooled minimum
    assert np.array_equal(tw.truncated_mean_target(qn, 1), [-1.0, 1.0])
    # the drop is from the POOL, not per net: E 2, H 2, dropped 2, net 0 = (10, 20), net 1 = (1, 2): both dropped values are net
    # 0's, the target is the mean of net 1's two = 1.5 (dropping one per net would give (10 + 1) / 2)
    assert tw.truncated_mean_target(np.array([[10.0, 20.0, 1.0, 2.0]]), 2)[0] == 1.5
    # duplicates straddling the cut: (1, 2, 2, 5), K = 2 -> 1.5 whichever 2 is kept
    assert tw.truncated_mean_target(np.array([[2.0, 5.0, 1.0, 2.0]]), 2)[0] == 1.5


def test_policy_seed_by_hand():
    """the policy ascends the mean over all T heads: the seed is -1 / (B T) everywhere, q_value the mean of the row means"""
    qa = np.array([[1.0, 3.0, 5.0, 7.0, 0.0, 2.0], [2.0, 2.0, 2.0, 2.0, 2.0, 8.0]])
    mean_q, seed = tw.policy_seed(qa)
    assert np.array_equal(mean_q, [3.0, 3.0]) and np.array_equal(seed, np.full((2, 6), -1.0 / 12.0))
    p = _case()
    met, _, _ = tw.policy_step(p["ps"], p["qs"], p["state"]["P"], p["state"]["Q"], p["state"]["la"][0], p["batch"][0][0].astype(np.float64),
                               p["eps2"], p["h"])
    import tqc_twin as tt
    from oracle import sac
    cm, cls, _, _ = sac.policy_forward(p["ps"], p["state"]["P"], p["batch"][0][0].astype(np.float64), -20.0, 2.0)
    ca, _ = sac.tanh_gaussian(cm, cls, p["eps2"])
    qa, _ = tt.critic_forward(p["qs"], p["state"]["Q"], 3, p["batch"][0][0].astype(np.float64), ca)
    assert qa.shape == (7, 6) and met["q_value/q_value"] == pytest.approx(qa.mean(axis=1).mean(), rel=1e-14)


# ------------------------------------------------------------------------------------------- the twin against torch.autograd
def _case(seed=3, **kw):
    args = dict(O=5, A=2, B=7, ph=[64], qh=[64], E=3, H=2, dropped=2, G=2)
    args.update(kw)
    p = tw.problem(seed, **args)
    rng = np.random.default_rng(seed + 1)
    G, B, A = args["G"], args["B"], args["A"]
    p["eps1"], p["eps2"] = rng.standard_normal((G, B, A)), rng.standard_normal((B, A))
    return p


def _update(p, st=None, lr_critic=LR, delta=0.0):
    cb = p["cbatch"] or (None, None)
    return tw.update(p["ps"], p["qs"], p["state"] if st is None else st, p["batch"], p["eps1"], p["eps2"], p["h"], LR, lr_critic, delta, LR, TAU,
                     cb[0], cb[1])


@pytest.mark.parametrize("Oc", [None, 4])
def test_twin_gradients_match_torch_autograd(Oc):
    """O 5, A 2, B 7, E 3, H 2, dropped 2, G 2, hidden [64]: step 1's critic gradient and -- with the critics left as they are
    (critic learning rate 0, so Adam and Polyak move nothing the policy step reads) -- the policy's and alpha's, at 1e-10"""
    p = _case(Oc=Oc)
    st = p["state"]
    new, met, g, ys = _update(p, lr_critic=0.0)
    assert np.array_equal(new["Q"], st["Q"])
    cb = p["cbatch"] or (None, None)
    b0 = tuple(x[0] for x in p["batch"])
    ql, gQ, pel, gP, gLA = tw.losses_torch(p["ps"], st["P"], p["qs"], st["Q"], st["QT"], st["la"][0], b0, p["eps1"][0], p["eps2"], p["h"],
                                           None if cb[0] is None else cb[0][0], None if cb[1] is None else cb[1][0])
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    assert rel(g["gq"][0], gQ) < 1e-10 and rel(g["gp"], gP) < 1e-10 and abs(g["ga"] - gLA) <= 1e-10 * abs(gLA)
    assert np.linalg.norm(gQ) > 0 and np.linalg.norm(gP) > 0
    assert met["loss/policy_loss"] + met["loss/entropy_loss"] == pytest.approx(pel, rel=1e-12)
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
    p1 = _case(G=1)
    n1, _, g1, _ = _update(p1)
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
    one = dict(p, batch=tuple(x[1:] for x in p["batch"]), eps1=p["eps1"][1:], h=dict(p["h"], q_update_steps=1),
               state=dict(st, QT=TAU * st["Q"] + (1 - TAU) * st["QT"]))
    _, _, g_one, ys_one = _update(one)
    assert np.array_equal(ys_one[0], ys0[1]) and np.array_equal(g_one["gq"][0], g0["gq"][1])
    _, metz, gz, _ = _update(p, lr_critic=0.0, delta=0.0)
    assert np.linalg.norm(gz["gp"] - g["gp"]) > 1e-9 * np.linalg.norm(g["gp"])
    assert metz["q_value/q_value"] != met["q_value/q_value"]


# ---------------------------------------------------------------------------------------------------------- the plugin
REFERENCE_DEFAULTS = dict(                                   # rl_x/algorithms/aqe/flax/default_config.py:9-28
    device="gpu", total_timesteps=1e9, learning_rate=3e-4, anneal_learning_rate=False, buffer_size=1e6, learning_starts=5000,
    batch_size=256, tau=0.005, gamma=0.99, ensemble_size=10, nr_heads_per_net=2, nr_dropped_q_values=4, q_update_steps=5,
    target_entropy="auto", log_std_min=-20, log_std_max=2, nr_hidden_units=256, logging_frequency=300, evaluation_frequency=-1,
    evaluation_episodes=10)


def test_aqe_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    from rlx_amd.runner.runner import Runner
    assert Runner._import_plugin("algorithms", "aqe.hip", ["rlx_amd"]) == "rlx_amd"
    import rlx_amd.algorithms.aqe.hip as plugin
    assert plugin.AQE_HIP == "aqe.hip"
    cfg = am.get_algorithm_config("aqe.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("aqe.hip")
    assert model.__name__ == "AQE" and model._NAME == "aqe.hip" and model._COUNTERS == ("nr_q_updates", "nr_policy_updates")
    from rlx_amd.algorithms.sac_ensemble import EnsembleSAC
    assert issubclass(model, EnsembleSAC)
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]
    from rlx_amd.hip import AqeHparams
    assert [n for n, _ in AqeHparams._fields_][-6:] == ["ensemble_size", "nr_heads_per_net", "nr_dropped_q_values", "q_update_steps",
                                                        "critic_states", "critic_next_states"]


@pytest.mark.parametrize("flags, msg", [
    (dict(device="cpu"), "MI355X"), (dict(ensemble_size=17), "aqe.hip: ensemble_size"), (dict(ensemble_size=0), "aqe.hip: ensemble_size"),
    (dict(nr_heads_per_net=0), "aqe.hip: nr_heads_per_net"), (dict(ensemble_size=13, nr_heads_per_net=10), "aqe.hip: .*at most 128"),
    (dict(nr_dropped_q_values=20), "aqe.hip: nr_dropped_q_values"), (dict(nr_dropped_q_values=-1), "aqe.hip: nr_dropped_q_values"),
    (dict(q_update_steps=0), "aqe.hip: q_update_steps"), (dict(q_update_steps=65), "aqe.hip: q_update_steps"),
    (dict(network_architecture="full_jit"), "flax networks"), (dict(enable_observation_normalization=True), "observation normalisation")])
def test_aqe_hip_refuses_what_it_cannot_run(flags, msg):
    """raised in front of anything that touches a device"""
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.aqe.hip  # noqa: F401
    cfg = am.get_algorithm_config("aqe.hip")
    for k, v in flags.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    config = sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
                environment=sn(seed=0, nr_envs=8))
    with pytest.raises(ValueError, match=msg):
        am.get_algorithm_model_class("aqe.hip")(config, None, None, "/nonexistent", None)


def test_aqe_hip_schedules():
    """aqe.py:83-99 are REDQ's: the critics' schedule divides by q_update_steps and counts critic steps; the plugin uses the REDQ
    plugin's two functions"""
    import rlx_amd.algorithms.aqe.hip.aqe as mod
    from rlx_amd.algorithms.redq.hip import redq
    assert mod.critic_lr_and_delta is redq.critic_lr_and_delta and mod.policy_lr is redq.policy_lr
    kw = dict(learning_rate=3e-4, nr_envs=4, learning_starts=100, total_timesteps=10100, q_update_steps=5)
    ref_q = lambda count: 3e-4 * (1.0 - ((count * 4) - 100) / ((10100 - 100) * 5))
    ref_p = lambda count: 3e-4 * (1.0 - ((count * 4) - 100) / (10100 - 100))
    lr, delta = mod.critic_lr_and_delta(35, anneal=True, **kw)
    assert lr == pytest.approx(ref_q(35), rel=1e-14) and lr + 3 * delta == pytest.approx(ref_q(38), rel=1e-12)
    assert mod.policy_lr(7, anneal=True, **kw) == pytest.approx(ref_p(7), rel=1e-14)
    assert mod.critic_lr_and_delta(35, anneal=False, **kw) == (3e-4, 0.0) and mod.policy_lr(7, anneal=False, **kw) == 3e-4
