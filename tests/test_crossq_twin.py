"""CPU: the batch-renormalisation twin (tests/crossq_twin.py) against float64 torch.autograd and hand-computed answers, and the
binding of the library's layer (rlx_brn_f32).

The autograd side restates batch_renorm.py:95-128 in torch with r and d detached (the reference's stop_gradient); the twin's
hand-written backward must agree to 1e-10 relative, not warmed and warmed, with both clips inactive and with r and d on either
edge.  Batch variances stay away from 0 there: at exactly 0 autograd gives NaN and the twin follows the library's documented rule."""
import ctypes

import numpy as np
import pytest
import torch

import crossq_twin as tw

BAR = 1e-10


def _rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-300))


def torch_brn_train(x, g, b, ra_mean, ra_var, cfg, warmed):
    mu = x.mean(0)
    v = torch.clamp((x * x).mean(0) - mu * mu, min=0)
    sig = torch.sqrt(ra_var + cfg.eps)
    r = torch.clamp(torch.sqrt(v + cfg.eps) / sig, 1 / cfg.r_max, cfg.r_max).detach()
    d = torch.clamp((mu - ra_mean) / sig, -cfg.d_max, cfg.d_max).detach()
    w = 1.0 if warmed else 0.0
    cm = mu - w * d * torch.sqrt(v) / r
    cv = v * (w / (r * r) + (1 - w))
    return (x - cm) * torch.rsqrt(cv + cfg.eps) * g + b


# what the running statistics are set to, per column, to put r / d where a case wants them: given the batch's mu and v,
# ra_var = (v + eps) / r_want^2 - eps and ra_mean = mu - d_want sqrt(ra_var + eps)
CLIP_CASES = {"inside": (1.3, 0.7), "r_low": (0.2, 0.5), "r_high": (4.0, -0.5), "d_low": (1.2, -7.0), "d_high": (0.8, 6.5)}


def make_case(name, M=9, D=6, seed=0):
    rng = np.random.default_rng([seed, M, D])
    x = rng.standard_normal((M, D)) * rng.uniform(0.5, 2.0, D) + rng.uniform(-2, 2, D)
    g, b, dY = 1 + 0.2 * rng.standard_normal(D), 0.3 * rng.standard_normal(D), rng.standard_normal((M, D))
    cfg = tw.BrnCfg()
    mu, v = tw.brn_batch_stats(x)
    r_want, d_want = CLIP_CASES[name]
    ra_var = (v + cfg.eps) / r_want ** 2 - cfg.eps
    ra_mean = mu - d_want * np.sqrt(ra_var + cfg.eps)
    return x, g, b, dY, ra_mean, ra_var, cfg


@pytest.mark.parametrize("warmed", [False, True])
@pytest.mark.parametrize("name", list(CLIP_CASES))
def test_layer_backward_matches_autograd(name, warmed):
    x, g, b, dY, ra_mean, ra_var, cfg = make_case(name)
    r_raw, d_raw, r, d = tw.brn_clips(*tw.brn_batch_stats(x), ra_mean, ra_var, cfg)
    r_want, d_want = CLIP_CASES[name]
    assert np.allclose(r_raw, r_want) and np.allclose(d_raw, d_want)                 # the case is what its name says
    assert np.all((r != r_raw) == (name.startswith("r_"))) and np.all((d != d_raw) == (name.startswith("d_")))
    y, cache, _, _ = tw.brn_train(x, g, b, ra_mean, ra_var, cfg, warmed)
    dX, dg, db = tw.brn_backward(dY, cache)
    tx, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, g, b))
    ty = torch_brn_train(tx, tg, tb, torch.tensor(ra_mean), torch.tensor(ra_var), cfg, warmed)
    ty.backward(torch.tensor(dY))
    for k, got, exp in (("y", y, ty.detach().numpy()), ("dX", dX, tx.grad.numpy()), ("dg", dg, tg.grad.numpy()), ("db", db, tb.grad.numpy())):
        assert _rel(got, exp) <= BAR, (name, warmed, k, _rel(got, exp))
    # the relu mask is the derivative of a ReLU in front of the layer
    tz = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    torch_brn_train(torch.relu(tz), tg.detach(), tb.detach(), torch.tensor(ra_mean), torch.tensor(ra_var), cfg, warmed).backward(torch.tensor(dY))
    xr = np.maximum(x, 0)
    _, cache_r, _, _ = tw.brn_train(xr, g, b, ra_mean, ra_var, cfg, warmed)
    assert _rel(tw.brn_backward(dY, cache_r, relu_mask=True)[0], tz.grad.numpy()) <= BAR


def test_eval_backward_matches_autograd():
    x, g, b, dY, ra_mean, ra_var, cfg = make_case("inside")
    y, cache = tw.brn_eval(x, g, b, ra_mean, ra_var, cfg)
    dX, dg, db = tw.brn_backward(dY, cache)
    tx, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, g, b))
    ty = (tx - torch.tensor(ra_mean)) * torch.rsqrt(torch.tensor(ra_var) + cfg.eps) * tg + tb
    ty.backward(torch.tensor(dY))
    for got, exp in ((y, ty.detach().numpy()), (dX, tx.grad.numpy()), (dg, tg.grad.numpy()), (db, tb.grad.numpy())):
        assert _rel(got, exp) <= BAR


def test_not_warmed_is_plain_batch_norm():
    x, g, b, _, ra_mean, ra_var, cfg = make_case("r_high")
    y, _, _, _ = tw.brn_train(x, g, b, ra_mean, ra_var, cfg, False)
    exp = (x - x.mean(0)) / np.sqrt(x.var(0) + cfg.eps) * g + b                      # eps 1e-3, whatever the running statistics
    assert _rel(y, exp) <= 1e-12


def test_eval_on_fresh_statistics():
    x, g, b, _, _, _, cfg = make_case("inside")
    y, _ = tw.brn_eval(x, g, b, np.zeros(6), np.ones(6), cfg)
    assert _rel(y, x * g / np.sqrt(1 + cfg.eps) + b) <= 1e-14
    assert abs(cfg.eps - 1e-3) < 1e-10                                               # sqrt(1.001), to float32's 1e-3


def test_running_statistics_after_one_pass():
    cfg = tw.BrnCfg()
    x = np.array([[1.0, 10.0], [3.0, 10.0], [5.0, 16.0]])
    _, _, m1, v1 = tw.brn_train(x, np.ones(2), np.zeros(2), np.zeros(2), np.ones(2), cfg, False)
    m = cfg.momentum
    assert np.allclose(m1, (1 - m) * np.array([3.0, 12.0]), rtol=1e-14)
    assert np.allclose(v1, m * 1.0 + (1 - m) * np.array([8.0 / 3.0, 8.0]), rtol=1e-13)
    # a warmed pass advances them in the same way: r and d do not enter
    _, _, m2, v2 = tw.brn_train(x, np.ones(2), np.zeros(2), np.zeros(2), np.ones(2), cfg, True)
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)


@pytest.mark.parametrize("warmed", [False, True])
def test_constant_column_is_finite_and_drops_the_sqrt_term(warmed):
    x, g, b, dY, ra_mean, ra_var, cfg = make_case("inside")
    x[:, 2] = 1.25                                                                   # exactly representable: v is exactly 0
    y, cache, _, _ = tw.brn_train(x, g, b, ra_mean, ra_var, cfg, warmed)
    assert cache["v"][2] == 0 and cache["t"][2] == 0
    dX, dg, db = tw.brn_backward(dY, cache)
    assert all(np.isfinite(a).all() for a in (y, dX, dg, db))
    dropped = tw.brn_backward(dY, cache, keep_sqrt_term=False)[0]
    assert np.array_equal(dX[:, 2], dropped[:, 2])
    others = [c for c in range(6) if c != 2]
    assert warmed == (not np.array_equal(dX[:, others], dropped[:, others]))         # elsewhere the term is kept


def test_binding_of_the_layer():
    from rlx_amd.hip import lib as L
    assert "rlx_brn_f32" in L.EXPORTED_SYMBOLS and hasattr(L.load_library(), "rlx_brn_f32")
    assert ctypes.sizeof(L.BrnConfig) == 5 * 4                                        # include/rlx_hip.h: rlx_brn_config
    c = L.brn_config(warmed=True)
    assert (c.momentum, c.eps, c.r_max, c.d_max, c.warmed) == (np.float32(0.99), np.float32(1e-3), 3.0, 5.0, 1)
    assert (L.BRN_EVAL_FWD, L.BRN_TRAIN_FWD, L.BRN_EVAL_BWD, L.BRN_TRAIN_BWD) == (0, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ the networks and the two updates
def torch_net(spec, p, stats, x, train, warmed, cfg):
    """net_forward restated in torch (float64) for autograd; p: a tensor that requires grad"""
    h = x
    for l in range(spec.L + 1):
        D, nxt = spec.dims[l], spec.dims[l + 1]
        g, b = p[spec.bn[l]:spec.bn[l] + D], p[spec.bn[l] + D:spec.bn[l] + 2 * D]
        m0, v0 = torch.tensor(stats[spec.st[l]:spec.st[l] + D]), torch.tensor(stats[spec.st[l] + D:spec.st[l] + 2 * D])
        y = torch_brn_train(h, g, b, m0, v0, cfg, warmed) if train else (h - m0) * torch.rsqrt(v0 + cfg.eps) * g + b
        z = y @ p[spec.W[l]:spec.W[l] + D * nxt].reshape(D, nxt) + p[spec.b[l]:spec.b[l] + nxt]
        h = torch.relu(z) if l < spec.L else z
    return h


def torch_sample(head, eps, ls_min, ls_max):
    A = head.shape[1] // 2
    ls = torch.clamp(head[:, A:], ls_min, ls_max)
    a = torch.tanh(head[:, :A] + torch.exp(ls) * eps)
    return a, (-0.5 * eps * eps - 0.5 * tw.LOG_2PI - ls - torch.log(1 - a * a + 1e-6)).sum(1)


@pytest.mark.parametrize("warmup", [100000, 0])
def test_whole_updates_match_autograd(warmup):
    c = tw.problem(3, 5, 2, 33, [64, 64], [64, 64], 2, warmup=warmup, stats_away=warmup == 0, dense_bias=1.0 if warmup == 0 else 0.0)
    ps, qs, st, h = c["ps"], c["qs"], c["state"], c["h"]
    cfg, B, E, A = tw.cfg_of(h), 33, 2, 2
    s, s2, a, r, term = (np.asarray(x, np.float64) for x in c["batch"])
    eps1, eps2 = (torch.tensor(e, dtype=torch.float64) for e in c["eps"])
    mid, m1, i1 = tw.critic_update(ps, qs, st, c["batch"], None, c["eps"][0], h)
    assert i1["warmed"] == (warmup == 0) and i1["vmin"] > 1e-6
    # the critic gradient: autograd through the joint pass of 2 B rows, the target under no_grad
    qp = torch.tensor(st["qp"], requires_grad=True)
    with torch.no_grad():
        a2, lp2 = torch_sample(torch_net(ps, torch.tensor(st["pp"]), st["ps"], torch.tensor(s2), False, False, cfg), eps1, -20.0, 2.0)
    x = torch.cat([torch.cat([torch.tensor(s), torch.tensor(a)], 1), torch.cat([torch.tensor(s2), a2], 1)], 0)
    q = torch.stack([torch_net(qs, qp[e * qs.n_params:(e + 1) * qs.n_params], st["qs"][e * qs.n_stats:(e + 1) * qs.n_stats], x, True, warmup == 0, cfg)[:, 0]
                     for e in range(E)], 1)
    y = (torch.tensor(r) + float(np.float32(0.99)) * (1 - torch.tensor(term)) * (q[B:].min(1).values - np.exp(st["la"][0]) * lp2)).detach()
    loss = ((q[:B] - y[:, None]) ** 2).mean()
    loss.backward()
    assert abs(float(loss.detach()) - m1["loss/q_loss"]) <= 1e-12 * max(1, abs(float(loss.detach())))
    assert _rel(i1["grad"], qp.grad.numpy()) <= BAR
    # Adam with b1 = 0.5, first step: m = (1 - b1) g, and the step is lr g / (|g| + eps) after the bias corrections
    g = qp.grad.numpy()
    assert _rel(mid["qm"], 0.5 * g) <= 1e-12 and _rel(mid["qv"], (1 - float(np.float32(0.999))) * g * g) <= 1e-12
    assert _rel(st["qp"] - mid["qp"], float(np.float32(1e-3)) * g / (np.abs(g) + float(np.float32(1e-8)))) <= 1e-6
    # the next-state rows carry gradient below the last BRN: zeroing it there changes the critic gradient by far more than 1e-3
    wrong = tw.critic_update(ps, qs, st, c["batch"], None, c["eps"][0], h, "zero_next_rows")[2]["grad"]
    assert _rel(wrong, i1["grad"]) > 1e-3
    assert _rel(tw.critic_update(ps, qs, st, c["batch"], None, c["eps"][0], h, "separate_halves")[2]["grad"], i1["grad"]) > 1e-3
    # the policy gradient: the policy in train mode, the critics in eval mode with the advanced statistics
    new, m2, i2 = tw.policy_update(ps, qs, mid, c["batch"], None, c["eps"][1], h)
    pp = torch.tensor(mid["pp"], requires_grad=True)
    act, lp = torch_sample(torch_net(ps, pp, mid["ps"], torch.tensor(s), True, warmup == 0, cfg), eps2, -20.0, 2.0)
    xq = torch.cat([torch.tensor(s), act], 1)
    qa = torch.stack([torch_net(qs, torch.tensor(mid["qp"][e * qs.n_params:(e + 1) * qs.n_params]), mid["qs"][e * qs.n_stats:(e + 1) * qs.n_stats], xq,
                                False, False, cfg)[:, 0] for e in range(E)], 1)
    ploss = (np.exp(mid["la"][0]) * lp - qa.min(1).values).mean()
    ploss.backward()
    assert abs(float(ploss.detach()) - m2["loss/policy_loss"]) <= 1e-12 and _rel(i2["grad"], pp.grad.numpy()) <= BAR
    ga = np.exp(mid["la"][0]) * (-float(lp.detach().mean()) - h["target_entropy"])
    assert abs(ga - m2["loss/entropy_loss"]) <= 1e-12
    assert (new["q_count"], new["pi_count"]) == (1, 1) and np.array_equal(new["qs"], mid["qs"]) and not np.array_equal(new["ps"], mid["ps"])


# ------------------------------------------------------------------- float32 with the column sums in double (FLOAT32 MODES, dsum)
def _gap_case(name):
    """(case, its float64 twin's (new, met)) of tests/test_gpu_crossq.py, whose figures and bars these tests use"""
    import test_gpu_crossq as m
    c = m.Case(name)
    return m, c, c.twin(c.state)[1:3]


def test_double_sums_leave_the_float64_twin_bit_identical():
    m, c, (new, met) = _gap_case("warm")
    _, new_d, met_d, _ = c.twin(c.state, dsum=True)
    assert all(np.array_equal(new[k], new_d[k]) for k in tw.STATE_KEYS) and met == met_d


def test_double_sum_layer_keeps_a_far_off_column():
    """a column of mean 50 and deviation 0.5 over 4096 rows: float32 sums lose its variance, double sums under float32 element-wise
    passes hold y, dX, dg, db to 1e-5 and the advanced statistics to 1e-6 -- the bars brn.hip is held to (tests/test_gpu_brn.py)"""
    rng = np.random.default_rng(7)
    M, D, cfg = 4096, 6, tw.BrnCfg()
    x = (50.0 + 0.5 * rng.standard_normal((M, D))).astype(np.float32)
    g, b, dY = (1 + 0.2 * rng.standard_normal(D)).astype(np.float32), (0.3 * rng.standard_normal(D)).astype(np.float32), \
        rng.standard_normal((M, D)).astype(np.float32)
    m0, v0 = np.full(D, 49.5, np.float32), np.full(D, 0.3, np.float32)
    f8 = lambda *a: [v.astype(np.float64) for v in a]
    y, cache, m1, v1 = tw.brn_train(*f8(x, g, b, m0, v0), cfg, True)
    exp = (y,) + tw.brn_backward(dY.astype(np.float64), cache) + (m1, v1)
    worst = {}
    for dsum in (False, True):
        y, cache, m1, v1 = tw.brn_train(x, g, b, m0, v0, cfg, True, dsum)
        got = (y,) + tw.brn_backward(dY, cache) + (m1, v1)
        assert all(a.dtype == np.float32 for a in got)
        worst[dsum] = [_rel(a, e) for a, e in zip(got, exp)]
    assert max(worst[True][:4]) <= 1e-5 and max(worst[True][4:]) <= 1e-6, worst[True]
    assert worst[False][0] > 1e-5 and worst[False][5] > 1e-5, worst[False]       # float sums miss both bars (y, the advanced variance)


@pytest.mark.parametrize("name", ["base", "warm"])
def test_double_sum_float32_is_within_half_of_every_bar(name):
    m, c, ref = _gap_case(name)
    gap = m.f32_gap(c, ref=ref)
    print(f"{name}: double-sum float32 twin against the float64 twin: " + " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
    bad = {k: (v, m.BARS[k]) for k, v in gap.items() if not v <= 0.5 * m.BARS[k]}
    assert not bad, bad


def test_double_sums_are_what_4096_rows_need():
    """why the mode exists: at 4096 rows the float32 twin's distance in the critics' first moments is the float column sums', which
    brn.hip does not take -- with them in double it is at least ten times closer, within half of every one-step bar, and the recorded
    F32_GAP leaves every bar of rows4096 at its one-step value"""
    m, c, ref = _gap_case("rows4096")
    naive, gap = m.f32_gap(c, dsum=False, ref=ref), m.f32_gap(c, ref=ref)
    print(f"rows4096 qm: float sums {naive['qm']:.2e}, double sums {gap['qm']:.2e}")
    assert naive["qm"] >= 10 * gap["qm"] and naive["qm"] > m.BARS["qm"]
    assert all(v <= 0.5 * m.BARS[k] for k, v in gap.items()), gap
    assert all(abs(v - m.F32_GAP["rows4096"][k]) <= 0.05 * m.BARS[k] for k, v in gap.items()), gap       # what is recorded is what this measures
    assert all(max(b, 2 * m.F32_GAP[n].get(k, 0.0)) == b for n in m.F32_GAP for k, b in m.BARS.items())


def test_key_chain_is_the_oracles():
    from oracle import prng
    key = prng.prng_key(5)
    for part in (True, False):
        k1, e1 = tw.key_chain(key, (7, 3), part)
        ks = prng.split(key, 2, part)
        assert np.array_equal(k1, ks[0]) and np.array_equal(e1, prng.normal(ks[1], (7, 3), partitionable=part))


def test_layout_counts_match_the_library():
    from rlx_amd.hip import lib as L
    lib = L.load_library()
    for in_dim, hidden, out in ((393, [2048, 2048], 1), (5, [64], 4), (7, [64, 192, 128], 1)):
        spec = tw.NetSpec(in_dim, hidden, out)
        d = L.mlp_desc(in_dim, hidden, out, 2, False, False)
        assert lib.rlx_crossq_param_count(ctypes.byref(d)) == spec.n_params and lib.rlx_crossq_stats_count(ctypes.byref(d)) == spec.n_stats
    assert ctypes.sizeof(L.CrossqHparams) == 16 * 4 + 2 * 4 + 2 * 8                  # include/rlx_hip.h: rlx_crossq_hparams


# ---------------------------------------------------------------------------------------------------------- the plugin
import types  # noqa: E402

REFERENCE_DEFAULTS = dict(                                   # rl_x/algorithms/crossq/flax/default_config.py
    device="gpu", total_timesteps=1e9, learning_rate=1e-3, anneal_learning_rate=False, policy_adam_b1=0.5, critic_adam_b1=0.5,
    buffer_size=10e6, learning_starts=5000, batch_size=256, gamma=0.99, ensemble_size=2, policy_delay=3, target_entropy="auto",
    log_std_min=-20, log_std_max=2, batch_renorm_momentum=0.99, batch_renorm_warmup_steps=100000, policy_nr_hidden_units=256,
    critic_nr_hidden_units=2048, logging_frequency=3000, evaluation_frequency=-1, evaluation_episodes=10)


def test_crossq_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    from rlx_amd.runner.runner import Runner
    assert Runner._import_plugin("algorithms", "crossq.hip", ["rlx_amd"]) == "rlx_amd"
    import rlx_amd.algorithms.crossq.hip as plugin
    assert plugin.CROSSQ_HIP == "crossq.hip"
    cfg = am.get_algorithm_config("crossq.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == REFERENCE_DEFAULTS and "tau" not in got
    model = am.get_algorithm_model_class("crossq.hip")
    from rlx_amd.algorithms.sac_ensemble import EnsembleSAC
    assert model.__name__ == "CrossQ" and issubclass(model, EnsembleSAC)
    assert model._COUNTERS[:2] == ("nr_q_updates", "nr_policy_updates") and "qtarget" not in model._STATE
    assert {"pstats", "qstats"} <= set(model._STATE)
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


@pytest.mark.parametrize("flags, msg", [
    (dict(device="cpu"), "MI355X"), (dict(network_architecture="full_jit"), "flax networks"),
    (dict(enable_observation_normalization=True), "observation normalisation"),
    (dict(critic_nr_hidden_units=96), "crossq.hip: critic_nr_hidden_units"), (dict(critic_nr_hidden_units=2112), "crossq.hip: critic_nr_hidden_units"),
    (dict(policy_nr_hidden_units=100), "crossq.hip: policy_nr_hidden_units"), (dict(ensemble_size=17), "crossq.hip: ensemble_size"),
    (dict(ensemble_size=0), "crossq.hip: ensemble_size"), (dict(policy_delay=0), "crossq.hip: policy_delay"),
    (dict(batch_size=1), "crossq.hip: batch_size"), (dict(batch_renorm_momentum=1.0), "crossq.hip: batch_renorm_momentum"),
    (dict(batch_renorm_warmup_steps=-1), "crossq.hip: batch_renorm_warmup_steps")])
def test_crossq_hip_refuses_what_it_cannot_run(flags, msg):
    """raised in front of anything that touches a device"""
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.crossq.hip  # noqa: F401
    cfg = am.get_algorithm_config("crossq.hip")
    for k, v in flags.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    config = sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
                environment=sn(seed=0, nr_envs=8))
    with pytest.raises(ValueError, match=msg):
        am.get_algorithm_model_class("crossq.hip")(config, None, None, "/nonexistent", None)


def test_policy_delay_rule_and_plugin_layout():
    """crossq.py:345: global_step % policy_delay == 0, global_step counting env steps; and the init layout is the twin's"""
    from rlx_amd.algorithms.crossq.hip.crossq import fresh_statistics, policy_is_due, with_batch_renorm
    assert [policy_is_due(g, 3) for g in (16, 32, 48, 96)] == [False, False, True, True]
    assert all(policy_is_due(g, 1) for g in range(5))
    spec = tw.NetSpec(3, [4, 2], 1)
    plain = np.arange(1, 3 * 4 + 4 + 4 * 2 + 2 + 2 * 1 + 1 + 1, dtype=np.float32)
    got = with_batch_renorm(plain, 3, [4, 2], 1)
    assert got.size == spec.n_params
    off = 0
    for l in range(spec.L + 1):
        D, nxt = spec.dims[l], spec.dims[l + 1]
        assert np.array_equal(got[spec.bn[l]:spec.bn[l] + 2 * D], np.concatenate([np.ones(D), np.zeros(D)]))
        assert np.array_equal(got[spec.W[l]:spec.b[l] + nxt], plain[off:off + D * nxt + nxt])
        off += D * nxt + nxt
    assert np.array_equal(fresh_statistics(3, [4, 2]), spec.fresh_stats())
