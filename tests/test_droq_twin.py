"""CPU: the DroQ twin (tests/droq_twin.py) -- hand-computed answers of the Dropout -> LayerNorm -> ReLU block, the gradients against
float64 torch.autograd with the masks as constants, REDQ's perturbation checks, the dependence of y on which mask array reaches
which pass -- the mask stream's two Python forms against each other, and the registration of the `droq.hip` plugin with the
reference's defaults."""
import types

import numpy as np
import pytest

import droq_twin as tw
from oracle import prng

LR, TAU = 3e-4, 0.005


# ------------------------------------------------------------------------------------------------------------ by hand
def test_block_by_hand():
    """one row, D = 4, rate 0.5 (keep 0.5), mask (1, 1, 0, 1), z = (1, 2, 7, 3), g = (1, 2, 1, 1), be = (0, 0, 1, -2), eps ~ 0:
    z' = (2, 4, 0, 6): the dropped 7 is gone and the others doubled; mean 3, E[z'^2] = 14, var 5, rstd = 1 / sqrt(5 + 1e-6);
    xhat = (-1, 1, -3, 3) rstd; H = relu(xhat g + be) = (0, 2 rstd, relu(1 - 3 rstd) = 0, relu(3 rstd - 2) = 0): 3 rstd = 1.34 < 2.
    Backward of dH = (1, 1, 1, 1): only unit 1 passes the ReLU: d = (0, 1, 0, 0), d scale = d xhat = (0, rstd', 0, 0) with rstd' =
    xhat_1, d bias = d; dxh = d g = (0, 2, 0, 0), m1 = 1/2, m2 = 2 xhat_1 / 4; dz' = rstd (dxh - m1 - xhat m2); dZ = dz' / keep on
    the kept units and EXACTLY 0 on the dropped one although dz'_2 = -0.2 rstd is not zero"""
    z = np.array([[1.0, 2.0, 7.0, 3.0]])
    mask = np.array([[True, True, False, True]])
    g, be = np.array([1.0, 2.0, 1.0, 1.0]), np.array([0.0, 0.0, 1.0, -2.0])
    H, c = tw.block_forward(z, mask, 0.5, g, be)
    assert np.array_equal(c["zd"], [[2.0, 4.0, 0.0, 6.0]])
    rstd = 1.0 / np.sqrt(5.0 + 1e-6)
    assert c["mu"][0, 0] == 3.0 and c["rstd"][0, 0] == pytest.approx(rstd, rel=1e-15)
    np.testing.assert_allclose(c["xhat"], [[-rstd, rstd, -3 * rstd, 3 * rstd]], rtol=1e-15)
    np.testing.assert_allclose(H, [[0.0, 2 * rstd, 0.0, 0.0]], rtol=1e-15)
    dz, dg, db = tw.block_backward(np.ones((1, 4)), c)
    np.testing.assert_allclose(dg, [0.0, rstd, 0.0, 0.0], rtol=1e-15)
    assert np.array_equal(db, [0.0, 1.0, 0.0, 0.0])
    m1, m2 = 0.5, 2.0 * rstd / 4.0
    dzd = rstd * (np.array([0.0, 2.0, 0.0, 0.0]) - m1 - np.array([-rstd, rstd, -3 * rstd, 3 * rstd]) * m2)
    assert dzd[2] == pytest.approx(-0.2 * rstd, rel=1e-5)          # rstd (1.5 rstd^2 - 1/2) with rstd^2 = 1 / 5
    np.testing.assert_allclose(dz, [[dzd[0] / 0.5, dzd[1] / 0.5, 0.0, dzd[3] / 0.5]], rtol=1e-14)
    assert dz[0, 2] == 0.0


def test_rate_zero_is_a_plain_layer_norm_relu_block():
    """rate 0: keep = 1 and an all-ones mask -- the block equals oracle/nets.py's LayerNorm + ReLU first layer, forward and backward"""
    from oracle import nets
    rng = np.random.default_rng(0)
    D, B = 8, 5
    spec = nets.MLPSpec(3, [D], 1, nets.ACT_RELU, True, False)
    p = rng.standard_normal(spec.n_params)
    x = rng.standard_normal((B, 3))
    out, cache = nets.forward(spec, p, x)
    L = spec.layers[0]
    z = x @ p[L["W"]:L["W"] + 3 * D].reshape(3, D) + p[L["b"]:L["b"] + D]
    assert tw.keep_prob(0.0) == 1.0
    H, c = tw.block_forward(z, np.ones((B, D), bool), tw.keep_prob(0.0), p[L["g"]:L["g"] + D], p[L["be"]:L["be"] + D])
    assert np.array_equal(H, cache["h"][0])
    d_out = rng.standard_normal((B, 1))
    g = nets.backward(spec, p, cache, d_out)
    dh = d_out @ p[spec.head["W"]:spec.head["W"] + D].reshape(D, 1).T
    dz, dg, db = tw.block_backward(dh, c)
    np.testing.assert_allclose(dg, g[L["g"]:L["g"] + D], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(db, g[L["be"]:L["be"] + D], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(dz.sum(axis=0), g[L["b"]:L["b"] + D], rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------ the mask stream
@pytest.mark.parametrize("rate", [0.01, 0.25, 0.9])
def test_mask_rows_equals_the_row_by_row_restatement(rate):
    key = prng.prng_key(31)
    for name in ("online", "target", "policy"):
        lay = tw.LAYOUTS[name](9)
        for j, E, l, L, D in ((0, 1, 0, 1, 64), (1, 2, 1, 3, 192), (15, 16, 2, 3, 64)):
            assert np.array_equal(tw.mask_rows(key, lay, j, E, l, L, 9, D, rate), tw.mask_stream(key, lay, j, E, l, L, 9, D, rate)), (name, j)


def test_mask_stream_addresses_and_share():
    """every address part matters (another layout, network, layer or scheme is another mask), the dropped share is the rate, and
    rate 0 draws nothing"""
    key, B, D = prng.prng_key(32), 16, 256
    base = tw.mask_stream(key, tw.LAYOUTS["online"](B), 0, 2, 0, 2, B, D, 0.25)
    assert abs((~base).mean() - 0.25) < 0.03
    on = tw.LAYOUTS["online"](B)
    for other in (tw.mask_stream(key, tw.LAYOUTS["target"](B), 0, 2, 0, 2, B, D, 0.25), tw.mask_stream(key, on, 1, 2, 0, 2, B, D, 0.25),
                  tw.mask_stream(key, on, 0, 2, 1, 2, B, D, 0.25), tw.mask_stream(key, on, 0, 2, 0, 2, B, D, 0.25, partitionable=False)):
        assert 0.3 < (other != base).mean() < 0.45                   # two independent masks differ on 2 * 0.25 * 0.75 of the units
    # the split COUNTS E and L reach the keys under the legacy scheme only: the partitionable split(key, n)[i] does not read n
    assert np.array_equal(tw.mask_stream(key, on, 0, 3, 0, 2, B, D, 0.25), base)
    leg = tw.mask_stream(key, on, 0, 2, 0, 2, B, D, 0.25, partitionable=False)
    assert 0.3 < (tw.mask_stream(key, on, 0, 3, 0, 2, B, D, 0.25, partitionable=False) != leg).mean() < 0.45
    assert 0.3 < (tw.mask_stream(key, on, 0, 2, 0, 3, B, D, 0.25, partitionable=False) != leg).mean() < 0.45
    # the target layout's row b is the online layout's row key one further: keys[4 + 3 b] against keys[3 + 3 b]
    assert tw.LAYOUTS["target"](B)[0] == tw.LAYOUTS["online"](B)[0] + 1
    assert tw.mask_stream(key, tw.LAYOUTS["online"](B), 0, 2, 0, 2, B, D, 0.0).all()
    # a lower rate keeps a superset: the same uniforms against a higher threshold
    low = tw.mask_stream(key, tw.LAYOUTS["online"](B), 0, 2, 0, 2, B, D, 0.01)
    assert (low | ~base).all() and low.sum() > base.sum()


# ------------------------------------------------------------------------------------------- the twin against torch.autograd
def _case(seed=3, rate=0.25, **kw):
    args = dict(O=5, A=2, B=7, ph=[64], qh=[64], E=3, M=2, G=2)
    args.update(kw)
    p = tw.problem(seed, rate=rate, **args)
    rng = np.random.default_rng(seed + 1)
    G, B, A, E, M = args["G"], args["B"], args["A"], args["E"], args["M"]
    p["eps1"], p["eps2"] = rng.standard_normal((G, B, A)), rng.standard_normal((B, A))
    p["subsets"] = np.array([rng.permutation(E)[:M] for _ in range(G)])
    keys = prng.split(prng.prng_key(seed), G + 1)
    p["masks"] = tw.update_masks(keys, B, args["qh"], E, M, rate, fast=True)
    return p


def _update(p, st=None, lr_critic=LR, delta=0.0, masks=None):
    cb = p["cbatch"] or (None, None)
    return tw.update(p["ps"], p["qs"], p["state"] if st is None else st, p["batch"], p["eps1"], p["eps2"], p["subsets"],
                     p["masks"] if masks is None else masks, p["h"], LR, lr_critic, delta, LR, TAU, cb[0], cb[1])


@pytest.mark.parametrize("Oc, qh", [(None, [64]), (4, [64, 128])])
def test_twin_gradients_match_torch_autograd(Oc, qh):
    """REDQ's small shape (O 5, A 2, B 7, E 3, M 2, G 2), masks as constants: step 0's critic gradient -- LayerNorm scale and bias
    included -- and, with the critics left as they are (critic learning rate 0), the policy's and alpha's, at 1e-10"""
    p = _case(Oc=Oc, qh=qh)
    st = p["state"]
    new, met, g, ys = _update(p, lr_critic=0.0)
    assert np.array_equal(new["Q"], st["Q"])
    cb = p["cbatch"] or (None, None)
    b0 = tuple(x[0] for x in p["batch"])
    m = p["masks"]
    ql, gQ, pel, gP, gLA = tw.losses_torch(p["ps"], st["P"], p["qs"], st["Q"], st["QT"], st["la"][0], b0, p["eps1"][0], p["eps2"], p["subsets"][0],
                                           m["online"][0], m["target"][0], m["policy"], p["h"], None if cb[0] is None else cb[0][0],
                                           None if cb[1] is None else cb[1][0])
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    assert rel(g["gq"][0], gQ) < 1e-10 and rel(g["gp"], gP) < 1e-10 and abs(g["ga"] - gLA) <= 1e-10 * abs(gLA)
    qs = p["qs"]
    L0 = qs.layers[0]
    ln = slice(L0["g"], L0["be"] + L0["out"])
    assert np.linalg.norm(gQ[ln]) > 0 and rel(g["gq"][0][ln], gQ[ln]) < 1e-10
    assert np.linalg.norm(gQ) > 0 and np.linalg.norm(gP) > 0
    assert met["loss/q_loss"] != ql or p["h"]["q_update_steps"] == 1      # q_loss is the mean over the G steps
    assert met["loss/policy_loss"] + met["loss/entropy_loss"] == pytest.approx(pel, rel=1e-12)
    assert met["gradients/policy_grad_norm"] == pytest.approx(np.linalg.norm(gP), rel=1e-10)
    # some masks of this case do drop units
    assert all(0 < (~x).sum() for net in m["online"][0] for x in net)


def test_twin_update_counters_means_adam_and_polyak():
    p = _case(G=3)
    st = p["state"]
    new, met, g, ys = _update(p, delta=-1e-5)
    assert (new["q_count"], new["pi_count"]) == (3, 1) and ys.shape == (3, 7)
    assert met["gradients/critic_grad_norm"] == pytest.approx(np.mean([np.linalg.norm(x) for x in g["gq"]]), rel=1e-14)
    np.testing.assert_allclose(new["pm"], 0.1 * g["gp"], rtol=1e-12)
    np.testing.assert_allclose(new["qm"], 0.1 * (0.81 * g["gq"][0] + 0.9 * g["gq"][1] + g["gq"][2]), rtol=1e-9, atol=1e-18)
    p1 = _case(G=1)
    n1, _, g1, _ = _update(p1)
    big = np.abs(g1["gq"][0]) > 1e-4
    np.testing.assert_allclose((n1["Q"] - p1["state"]["Q"])[big], -LR * np.sign(g1["gq"][0][big]), rtol=1e-3)
    # Polyak runs over the whole flat vector, LayerNorm parameters included
    np.testing.assert_allclose(n1["QT"], TAU * n1["Q"] + (1 - TAU) * p1["state"]["QT"], rtol=1e-14)
    L0 = p1["qs"].layers[0]
    ln = slice(L0["g"], L0["be"] + L0["out"])
    assert not np.array_equal(n1["Q"][ln], p1["state"]["Q"][ln]) and not np.array_equal(n1["QT"][ln], p1["state"]["QT"][ln])
    assert not np.array_equal(n1["la"], p1["state"]["la"]) and not np.array_equal(new["P"], st["P"])


def test_every_step_sees_the_one_before():
    """REDQ's perturbation check: with step 1's learning rate zeroed step 2's y and gradient change, step 1's do not; step 2 of the
    zeroed run equals a single step on batch 1 (and step 1's masks) from the state step 1's Polyak left; the policy step reads the
    critics from after step G"""
    p = _case(G=2)
    new, met, g, ys = _update(p)
    new0, met0, g0, ys0 = _update(p, lr_critic=0.0, delta=LR)
    assert np.array_equal(ys0[0], ys[0]) and np.array_equal(g0["gq"][0], g["gq"][0])
    assert np.abs(ys0[1] - ys[1]).max() > 1e-9 and np.linalg.norm(g0["gq"][1] - g["gq"][1]) > 1e-9 * np.linalg.norm(g["gq"][1])
    st, m = p["state"], p["masks"]
    one = dict(p, batch=tuple(x[1:] for x in p["batch"]), eps1=p["eps1"][1:], subsets=p["subsets"][1:], h=dict(p["h"], q_update_steps=1),
               state=dict(st, QT=TAU * st["Q"] + (1 - TAU) * st["QT"]),
               masks={"online": m["online"][1:], "target": m["target"][1:], "policy": m["policy"]})
    _, _, g_one, ys_one = _update(one)
    assert np.array_equal(ys_one[0], ys0[1]) and np.array_equal(g_one["gq"][0], g0["gq"][1])
    _, metz, gz, _ = _update(p, lr_critic=0.0, delta=0.0)
    assert np.linalg.norm(gz["gp"] - g["gp"]) > 1e-9 * np.linalg.norm(g["gp"])
    assert metz["q_value/q_value"] != met["q_value/q_value"]


def test_swapping_online_and_target_masks_changes_y():
    """y is computed under the TARGET masks and the gradient under the ONLINE ones: exchanging the two arrays changes both; the
    policy step's masks reach only the policy step"""
    p = _case(G=1)
    _, met, g, ys = _update(p)
    sw = tw.swap_online_target(p["masks"], 2)
    assert np.array_equal(sw["target"][0][0][0], p["masks"]["online"][0][0][0])
    _, mets, gs, yss = _update(p, masks=sw)
    assert np.abs(yss - ys).max() > 1e-6 and np.linalg.norm(gs["gq"][0] - g["gq"][0]) > 1e-6 * np.linalg.norm(g["gq"][0])
    ones = dict(p["masks"], policy=[[np.ones_like(x) for x in net] for net in p["masks"]["policy"]])
    _, meto, go, yso = _update(p, masks=ones)
    assert np.array_equal(yso, ys) and np.array_equal(go["gq"][0], g["gq"][0])
    assert meto["q_value/q_value"] != met["q_value/q_value"] and not np.array_equal(go["gp"], g["gp"])


def test_rate_zero_masks_are_all_ones_and_float32_twin_runs():
    p = _case(rate=0.0)
    assert all(x.all() for net in p["masks"]["policy"] for x in net)
    st32 = {k: (v.astype(np.float32) if k in tw.STATE_KEYS else v) for k, v in p["state"].items()}
    new32, _, _, _ = _update(p, st=st32)
    new, _, _, _ = _update(p)
    assert new32["Q"].dtype == np.float32 and np.abs(new32["Q"] - new["Q"]).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------- the plugin
REFERENCE_DEFAULTS = dict(                                   # rl_x/algorithms/droq/flax/default_config.py:9-28
    device="gpu", total_timesteps=1e9, learning_rate=3e-4, anneal_learning_rate=False, buffer_size=1e6, learning_starts=5000,
    batch_size=256, tau=0.005, gamma=0.99, ensemble_size=2, in_target_minimization_size=2, dropout_rate=0.01, q_update_steps=20,
    target_entropy="auto", log_std_min=-20, log_std_max=2, nr_hidden_units=256, logging_frequency=100, evaluation_frequency=-1,
    evaluation_episodes=10)


def test_droq_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    from rlx_amd.runner.runner import Runner
    assert Runner._import_plugin("algorithms", "droq.hip", ["rlx_amd"]) == "rlx_amd"
    import rlx_amd.algorithms.droq.hip as plugin
    assert plugin.DROQ_HIP == "droq.hip"
    cfg = am.get_algorithm_config("droq.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("droq.hip")
    assert model.__name__ == "DroQ"
    from rlx_amd.algorithms.redq.hip.redq import REDQ
    assert issubclass(model, REDQ)
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


@pytest.mark.parametrize("flags, msg", [
    (dict(device="cpu"), "MI355X"), (dict(dropout_rate=1.0), "droq.hip: dropout_rate"), (dict(dropout_rate=-0.1), "droq.hip: dropout_rate"),
    (dict(nr_hidden_units=832), "droq.hip: nr_hidden_units"), (dict(nr_hidden_units=100), "droq.hip: nr_hidden_units"),
    (dict(ensemble_size=17), "droq.hip: ensemble_size"), (dict(in_target_minimization_size=3), "droq.hip: in_target_minimization_size"),
    (dict(q_update_steps=0), "droq.hip: q_update_steps"), (dict(batch_size=2 ** 30), "droq.hip: batch_size"),
    (dict(network_architecture="full_jit"), "flax networks"), (dict(enable_observation_normalization=True), "observation normalisation")])
def test_droq_hip_refuses_what_it_cannot_run(flags, msg):
    """raised in front of anything that touches a device"""
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.droq.hip  # noqa: F401
    cfg = am.get_algorithm_config("droq.hip")
    for k, v in flags.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    config = sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
                environment=sn(seed=0, nr_envs=8))
    with pytest.raises(ValueError, match=msg):
        am.get_algorithm_model_class("droq.hip")(config, None, None, "/nonexistent", None)


def test_layer_norm_layout_of_the_plugin_init():
    """_with_layer_norm puts scale 1 and bias 0 after every hidden bias and keeps every other entry: the twin's layout"""
    from rlx_amd.algorithms.droq.hip.droq import _with_layer_norm
    n_in, hidden = 3, [4, 2]
    plain = np.arange(1, 3 * 4 + 4 + 4 * 2 + 2 + 2 * 1 + 1 + 1, dtype=np.float32)
    got = _with_layer_norm(plain, n_in, hidden, 1)
    qs = tw.CriticSpec(n_in, hidden, 1)
    assert got.size == qs.n_params
    off = 0
    for L in qs.layers:
        n = L["in"] * L["out"] + L["out"]
        assert np.array_equal(got[L["W"]:L["W"] + n], plain[off:off + n])
        assert np.array_equal(got[L["g"]:L["g"] + L["out"]], np.ones(L["out"])) and np.array_equal(got[L["be"]:L["be"] + L["out"]], np.zeros(L["out"]))
        off += n
    assert np.array_equal(got[qs.head["W"]:], plain[off:])
