"""CPU: REPPO's float64 twin (tests/reppo_twin.py) against the fixture produced by the reference's own modules and closures
(tests/golden/reppo_reference.npz, regenerated bit for bit when the reference checkout is present), layouts and parameter counts
against the library's ctypes view, closed forms, and the `reppo.hip` plugin's registered defaults and refusals."""
import math
import os

import numpy as np
import pytest
import torch

import reppo_twin as tw

REF = os.environ.get("RLX_REFERENCE", "/root/reference")


def test_layouts_and_param_counts():
    LP, LQ = tw.policy_layout(17, 6, 512), tw.critic_layout(20, 6, 512, 151)
    assert LP["n"] == (17 * 512 + 2 * 512) + (512 * 512 + 2 * 512) + (512 * 12 + 12) + 2
    assert LQ["n"] == (26 * 512 + 2 * 512) + (512 * 512 + 512) + 2 * (512 * 512 + 2 * 512) + (512 * 151 + 151) + (512 * 513 + 513) + 151
    p, q = tw.make_params(0, 17, 20, 6, 512, 512, 151, -100.0, 100.0)
    assert p.size == LP["n"] and q.size == LQ["n"] and p.dtype == np.float32
    assert p[LP["coef"]] == np.float32(math.log(0.01)) and np.all(q[LQ["c0"]["g"]:LQ["c0"]["g"] + 512] == 1.0)
    assert abs(q[LQ["zd"]:].sum() - 1.0) < 1e-5


def test_library_descriptor_and_hparams_layout():
    import ctypes
    from rlx_amd.hip import ReppoDesc, ReppoHparams, reppo_desc
    from rlx_amd.hip import lib as L
    assert ctypes.sizeof(ReppoDesc) == 24 and ctypes.sizeof(ReppoHparams) == 13 * 4
    d = reppo_desc(17, 20, 6, 512, 512, 151)
    assert (d.policy_obs_dim, d.critic_obs_dim, d.act_dim, d.nr_bins) == (17, 20, 6, 151)
    for name in ("rlx_reppo_param_count", "rlx_reppo_update_f32", "rlx_reppo_policy_step_f32", "rlx_reppo_critic_step_f32",
                 "rlx_reppo_evaluate_next_f32", "rlx_reppo_act_f32", "rlx_reppo_td_lambda_f32", "rlx_reppo_obs_norm_update_f32",
                 "rlx_reppo_obs_norm_apply_f32"):
        assert name in L.EXPORTED_SYMBOLS
    if os.path.exists(L.library_path()):
        lib = L.load_library()
        assert lib.rlx_reppo_param_count(ctypes.byref(d), 0) == tw.policy_layout(17, 6, 512)["n"]
        assert lib.rlx_reppo_param_count(ctypes.byref(d), 1) == tw.critic_layout(20, 6, 512, 151)["n"]
        assert lib.rlx_reppo_param_count(ctypes.byref(d), 2) == -1


def test_sampled_log_prob_equals_log_prob_at_the_sample():
    rng = np.random.default_rng(1)
    loc, ls, e = (torch.tensor(rng.standard_normal((50, 4)) * s) for s in (0.5, 0.3, 1.0))
    a, lp = tw.sample_and_log_prob(loc, ls, e, 0.0)
    assert torch.allclose(lp, tw.log_prob(loc, ls, a, 0.0), rtol=0, atol=1e-7)


def test_td_lambda_closed_forms():
    rng = np.random.default_rng(2)
    sr, nv = rng.standard_normal((9, 5)), rng.standard_normal((9, 5))
    z = np.zeros((9, 5))
    assert np.allclose(tw.td_lambda(sr, nv, z, z, 0.9, 0.0), sr + 0.9 * nv, rtol=0, atol=1e-14)
    tr = np.ones((9, 5))
    assert np.allclose(tw.td_lambda(sr, nv, z, tr, 0.9, 0.7), sr + 0.9 * nv, rtol=0, atol=1e-14)
    assert np.allclose(tw.td_lambda(sr, nv, tr, z, 0.9, 0.7), sr, rtol=0, atol=1e-14)


def test_obs_norm_count_is_float32():
    m, v, c = np.zeros(3, np.float32), np.ones(3, np.float32), np.float32(1e-4)
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    m, v, c = tw.obs_norm_update(m, v, c, x)
    assert c.dtype == np.float32 and c == np.float32(np.float32(1e-4) + np.float32(4))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "rl_x/algorithms/reppo/pytorch")), reason="needs the reference checkout")
@pytest.mark.parametrize("Hp,Hc,NB,v", [(64, 64, 21, 10.0), (128, 64, 151, 100.0), (64, 192, 65, 100.0)],
                         ids=["h64_v10", "hp128_hc64_v100", "hp64_hc192_v100"])
def test_networks_match_the_reference_modules(Hp, Hc, NB, v):
    """the twin's network forward passes against the reference's Policy / Critic modules in float64 (the sampler, the losses and
    the normaliser are pinned by the fixture tests below)"""
    import sys
    import types
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_reference_golden import load_by_path
    sys.path.insert(0, REF)
    pol = load_by_path("rl_x/algorithms/reppo/pytorch/policy.py", "ref_reppo_policy")
    cri = load_by_path("rl_x/algorithms/reppo/pytorch/critic.py", "ref_reppo_critic")
    O, A = 7, 2
    sp = types.SimpleNamespace
    env = sp(single_action_space=sp(low=-np.ones(A, np.float32), high=np.ones(A, np.float32), shape=(A,)),
             single_observation_space=sp(shape=(O,)))
    P = pol.Policy(env, Hp, 0.0, 0.05, 0.02, np.arange(O), "cpu").double()
    C = cri.Critic(env, Hc, NB, -v, v, np.arange(O), "cpu").double()
    for m in list(P.modules()) + list(C.modules()):
        if isinstance(m, torch.nn.RMSNorm):
            m.eps = tw.RMS_EPS
    p, q = tw.make_params(3, O, O, A, Hp, Hc, NB, -v, v, 0.05, 0.02)
    LP, LQ = tw.policy_layout(O, A, Hp), tw.critic_layout(O, A, Hc, NB)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))

    def load(seq_lins, L, names, flat):
        for lin, k in zip(seq_lins, names):
            e = L[k]
            lin.weight.data.copy_(t(flat[e["W"]:e["W"] + e["in"] * e["out"]].reshape(e["in"], e["out"]).T))
            lin.bias.data.copy_(t(flat[e["b"]:e["b"] + e["out"]]))
    lins = lambda s: [m for m in s if isinstance(m, torch.nn.Linear)]
    load(lins(P.torso) + [P.head], LP, ("l0", "l1", "head"), p)
    load(lins(C.encoder) + lins(C.critic_head) + lins(C.pred_head), LQ, ("e0", "e1", "c0", "c1", "p0", "p1"), q)
    with torch.no_grad():
        P.log_entropy_coefficient.copy_(t(p[LP["coef"]:LP["coef"] + 1]))
        P.log_kl_coefficient.copy_(t(p[LP["coef"] + 1:]))
        C.zero_distribution.copy_(t(q[LQ["zd"]:]))
    assert np.array_equal(np.asarray(C.zero_distribution.detach().numpy(), np.float32), tw.zero_distribution(NB, -v, v))
    rng = np.random.default_rng(4)
    x, e = t(rng.standard_normal((9, O))), t(rng.standard_normal((9, A)))
    with torch.no_grad():
        loc, ls = P(x)
        tl, tls = tw.policy_fwd(t(p), LP, x)
        assert torch.allclose(loc, tl, rtol=1e-12, atol=1e-14) and torch.allclose(ls, tls, rtol=1e-12, atol=1e-14)
        a = torch.tanh(loc + ls.exp() * e)
        f, lg, pf, pr = C(x, a)
        F, lg2, pred = tw.critic_fwd(t(q), LQ, torch.cat([x, a], -1))
        assert torch.allclose(f, F, rtol=1e-12, atol=1e-14) and torch.allclose(lg, lg2, rtol=1e-12, atol=1e-13)
        assert torch.allclose(torch.cat([pr, pf], -1), pred, rtol=1e-12, atol=1e-13)


GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reppo_reference.npz")
LR = 3e-4


def _check_sampled(z, name, full, tol=1e-12):
    idx = z[name + "_idx"]
    assert abs(np.linalg.norm(full) - z[name + "_norm"]) <= tol * z[name + "_norm"], name
    assert np.linalg.norm(full[idx] - z[name + "_val"]) <= tol * np.linalg.norm(z[name + "_val"]), name


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_fixture_is_inputs_and_outputs_only():
    z = np.load(GOLDEN)
    assert str(z["source"]).startswith("reference:rl_x/algorithms/reppo/pytorch")
    assert not os.path.basename(GOLDEN).startswith("reference_")
    assert int(z["n_cases"]) == 4


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_twin_reproduces_the_reference_fixture(c):
    z = np.load(GOLDEN)
    k = "c%d_" % c
    g = lambda n: z[k + n]
    fc = tw.fixture_case(z, c)
    hp, p, q, old_p, LP, LQ = (fc[n] for n in ("hp", "p", "q", "old_p", "LP", "LQ"))
    s, s2 = g("states"), g("next_states")
    F, v, sr = tw.evaluate_next(p, LP, q, LQ, s2, s2, g("rewards"), g("eps_eval"), hp)
    assert _rel(F, g("eval_next_features")) < 1e-12 and _rel(v, g("eval_next_value")) < 1e-12 and _rel(sr, g("eval_soft_reward")) < 1e-12
    batch = (s, g("actions"), g("targets"), g("rewards"), g("next_features"), g("terms"), g("truncs"))
    assert g("terms").sum() > 0 and g("truncs").sum() > 0
    zq = np.zeros(q.size)
    rq, rm, rv, cm, gq = tw.critic_step(q, zq, zq, 1, LR, LQ, batch, hp)
    assert np.all(np.abs(cm - g("critic_metrics")) <= 1e-12 * np.maximum(np.abs(g("critic_metrics")), 1.0))
    clip = lambda grad, norm: grad * min(1.0, hp["max_grad_norm"] / (norm + 1e-6))     # clip_grad_norm_ clips .grad in place
    _check_sampled(z, k + "gcritic", clip(gq, cm[4]))
    _check_sampled(z, k + "qparams_after", rq)
    _check_sampled(z, k + "qv_after", rv)
    zp = np.zeros(p.size)
    rp, _, _, pm, gp, kl = tw.policy_step(p, zp, zp, old_p, rq, 1, LR, LP, LQ, s, s, g("eps_new"), g("eps_old"), hp)
    assert np.all(np.abs(pm - g("policy_metrics")) <= 1e-12 * np.maximum(np.abs(g("policy_metrics")), 1.0))
    _check_sampled(z, k + "gpolicy", clip(gp, pm[8]))
    _check_sampled(z, k + "pparams_after", rp)
    inside = kl < hp["kl_bound"]
    if c == 0:
        assert inside.all()
    else:
        assert 0 < inside.sum() < len(kl)
        assert np.min(np.abs(kl - hp["kl_bound"])) > 1e-4          # every row far from the bound next to float32 error
    if c == 2:
        assert g("critic_metrics")[4] > hp["max_grad_norm"] and g("policy_metrics")[8] > hp["max_grad_norm"]
    if c == 3:      # the regimes this case is there for
        assert (fc["Hp"], fc["Hc"], fc["NB"], hp["v_max"]) == (128, 64, 151, 100.0) and -hp["v_min"] == hp["v_max"]
        assert hp["policy_min_std"] > 0 and hp["auxiliary_loss_coefficient"] != 1.0
        t = g("targets")
        assert (t > hp["v_max"]).sum() >= 2 and (t < hp["v_min"]).sum() >= 2 and (t == hp["v_max"]).any() and (t == hp["v_min"]).any()
    assert _rel(tw.td_lambda(g("td_soft_rewards"), g("td_next_values"), g("td_terms"), g("td_truncs"), 0.99, 0.95), g("td_targets")) < 1e-12


def test_twin_normaliser_reproduces_the_reference():
    z = np.load(GOLDEN)
    m, v, cnt = np.zeros(5, np.float32), np.ones(5, np.float32), np.float32(1e-4)
    for x in z["norm_inputs"]:
        m, v, cnt = tw.obs_norm_update(m, v, cnt, x)
    assert np.array_equal(m, z["norm_mean"]) and np.array_equal(v, z["norm_var"]) and cnt == z["norm_count"]
    out = (z["norm_inputs"][-1] - m) / np.sqrt(v + np.float32(1e-8))
    assert np.array_equal(out.astype(np.float32), z["norm_out"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "rl_x/algorithms/reppo/pytorch")), reason="needs the reference checkout")
def test_fixture_regenerates_bit_for_bit(tmp_path, monkeypatch):
    import importlib.util
    monkeypatch.setenv("RLX_GOLDEN_OUT", str(tmp_path))
    path = os.path.join(os.path.dirname(__file__), "golden", "make_reppo_golden.py")
    spec = importlib.util.spec_from_file_location("make_reppo_golden_t", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        mod.make_reppo()
    finally:
        torch.set_default_dtype(torch.float32)
    za, zb = np.load(GOLDEN), np.load(os.path.join(str(tmp_path), "reppo_reference.npz"))
    assert sorted(za.files) == sorted(zb.files)
    for k in za.files:
        x, y = za[k], zb[k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


# reppo/pytorch/default_config.py; the plugin differs in compile_mode (nothing is traced) and bf16_mixed_precision_training (fp32),
# and adds threefry_partitionable (its counter RNG)
REFERENCE_DEFAULTS = dict(
    device="gpu", compile_mode="reduce-overhead", bf16_mixed_precision_training=True, total_timesteps=1000000000, learning_rate=3e-4,
    anneal_learning_rate=False, nr_steps=128, nr_epochs=4, nr_minibatches=128, gamma=0.99, gae_lambda=0.95, max_grad_norm=0.5,
    policy_hidden_dim=512, critic_hidden_dim=512, policy_min_std=0.0, nr_bins=151, v_min=-100.0, v_max=100.0, init_kl_coefficient=0.01,
    kl_bound=0.1, init_entropy_coefficient=0.01, target_entropy_multiplier=0.5, auxiliary_loss_coefficient=1.0, nr_kl_samples=16,
    normalize_observation=True, evaluation_frequency=-1, evaluation_episodes=10)
DIFFERENT = dict(compile_mode="none", bf16_mixed_precision_training=False)


def test_reppo_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.reppo.hip as plugin
    assert plugin.REPPO_HIP == "reppo.hip"
    cfg = am.get_algorithm_config("reppo.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == dict(REFERENCE_DEFAULTS, **DIFFERENT)
    path = os.path.join(REF, "rl_x", "algorithms", "reppo", "pytorch", "default_config.py")
    if os.path.exists(path):
        import sys
        import types
        ml = types.ModuleType("ml_collections")

        class Cfg(dict):
            __getattr__ = dict.__getitem__

            def __setattr__(self, k, v):
                self[k] = v
        ml.config_dict = types.SimpleNamespace(ConfigDict=Cfg)
        saved, ns = sys.modules.get("ml_collections"), {}
        sys.modules["ml_collections"] = ml
        try:
            exec(compile(open(path).read(), path, "exec"), ns)
        finally:
            if saved is None:
                del sys.modules["ml_collections"]
            else:
                sys.modules["ml_collections"] = saved
        ref = dict(ns["get_config"]("reppo.pytorch"))
        ref.pop("name")
        assert ref == REFERENCE_DEFAULTS
    model = am.get_algorithm_model_class("reppo.hip")
    assert model.__name__ == "REPPO"
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


def _config(**alg):
    import types
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.reppo.hip  # noqa: F401
    cfg = am.get_algorithm_config("reppo.hip")
    for k, v in alg.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    return sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
              environment=sn(seed=0, nr_envs=8))


def _env(interface):
    import types
    from rlx_amd.environments.data_interface_type import DataInterfaceType
    return types.SimpleNamespace(general_properties=types.SimpleNamespace(data_interface_type=DataInterfaceType[interface]))


@pytest.mark.parametrize("flags, interface, msg", [(dict(bf16_mixed_precision_training=True), "TORCH", "fp32"),
                                                   (dict(device="cpu"), "TORCH", "MI355X"),
                                                   (dict(), "NUMPY", "TORCH data-interface"),
                                                   (dict(nr_minibatches=7), "TORCH", "divisible")])
def test_reppo_hip_refuses_what_it_does_not_emulate(flags, interface, msg):
    from rlx_amd.algorithms.reppo.hip.reppo import REPPO
    with pytest.raises(ValueError, match=msg):
        REPPO(_config(**flags), _env(interface), None, "/nonexistent", None)


def test_plugin_initialisation_matches_the_twin_layout():
    from rlx_amd.algorithms.reppo.hip.reppo import init_params
    p, q = init_params(np.random.default_rng(0), 17, 20, 6, 128, 64, 51, -100.0, 100.0, 0.01, 0.02)
    LP, LQ = tw.policy_layout(17, 6, 128), tw.critic_layout(20, 6, 64, 51)
    assert p.size == LP["n"] and q.size == LQ["n"]
    assert p[LP["coef"]] == np.float32(math.log(0.01)) and p[LP["coef"] + 1] == np.float32(math.log(0.02))
    assert np.all(p[LP["l1"]["g"]:LP["l1"]["g"] + 128] == 1.0) and np.all(q[LQ["p0"]["g"]:LQ["p0"]["g"] + 64] == 1.0)
    assert np.array_equal(q[LQ["zd"]:], tw.zero_distribution(51, -100.0, 100.0))
    b = 1.0 / np.sqrt(20 + 6)
    w = q[LQ["e0"]["W"]:LQ["e0"]["W"] + 26 * 64]
    assert np.abs(w).max() <= b and np.abs(w).max() > 0.9 * b
