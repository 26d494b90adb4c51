"""CPU: tests/td3_twin.py (the numpy restatement of TD3's and DDPG's updates; the reference's are JAX only: PARITY UNPINNED) pinned
by hand-computed answers and by float64 torch.autograd."""
import numpy as np
import pytest

import td3_twin as tw
from oracle import nets, prng

LR, TAU = 3e-4, 0.005


def _problem(E=2, Oc=None, seed=3):
    return tw.problem(seed, 6, 3, 19, [16, 16], [16, 16], E, Oc, head_scale=3.0)     # (x 3: tanh near +-1 on some rows)


def _noise(p, seed=5):
    B, A = p["batch"][2].shape
    return np.random.default_rng(seed).standard_normal((B, A)) * 2.0      # (x 2: a good share of the rows beyond the inner clip)


@pytest.mark.parametrize("Oc", [None, 4])
def test_td3_gradients_match_torch_autograd(Oc):
    p = _problem(2, Oc)
    st, cb = p["state"], p["cbatch"] or (None, None)
    noise = _noise(p)
    b = tuple(np.asarray(x, np.float64) for x in p["batch"])
    c = lambda x: None if x is None else np.asarray(x, np.float64)
    ql, gq, aux = tw.critic_grads(p["ps"], p["qs"], st["PT"], st["Q"], st["QT"], b, noise, p["h"], c(cb[0]), c(cb[1]))
    met, gp, _ = tw.policy_grads(p["ps"], p["qs"], st["P"], st["Q"], b[0], p["h"], c(cb[0]))
    tql, tgq, tpl, tgp = tw.losses_torch(p["ps"], p["qs"], st["P"], st["PT"], st["Q"], st["QT"], p["batch"], noise, p["h"], cb[0], cb[1])
    assert ql == pytest.approx(tql, rel=1e-12) and met["loss/policy_loss"] == pytest.approx(tpl, rel=1e-12)
    assert np.abs(gq - tgq).max() <= 1e-12 * np.abs(tgq).max() and np.abs(gp - tgp).max() <= 1e-12 * np.abs(tgp).max()
    assert np.linalg.norm(gq) > 0 and np.linalg.norm(gp) > 0
    # both clips act in this batch: some noise beyond the inner clip, some smoothed action at +-1
    assert (np.abs(noise * 0.2) > 0.5).any() and (np.abs(aux["next_action"]) == 1.0).any()
    assert met["q_value/q_value"] == -met["loss/policy_loss"]


def test_ddpg_joint_gradients_match_torch_autograd():
    p = _problem(1)
    st = p["state"]
    new, met, aux = tw.ddpg_step(p["ps"], p["qs"], st, p["batch"], p["h"], LR, LR, TAU)
    tql, tgq, tpl, tgp = tw.losses_torch(p["ps"], p["qs"], st["P"], st["PT"], st["Q"], st["QT"], p["batch"], None, p["h"], joint=True)
    assert met["loss/q_loss"] == pytest.approx(tql, rel=1e-12) and met["loss/policy_loss"] == pytest.approx(tpl, rel=1e-12)
    assert np.abs(aux["gq"] - tgq).max() <= 1e-12 * np.abs(tgq).max() and np.abs(aux["gp"] - tgp).max() <= 1e-12 * np.abs(tgp).max()
    # the policy's gradient flows through the critic BEFORE its step: the critics of the TD3 order (after the step) give another one
    after, _, _ = tw.critic_step(p["ps"], p["qs"], st, p["batch"], None, p["h"], LR)
    _, gp_after, _ = tw.policy_grads(p["ps"], p["qs"], st["P"], after["Q"], np.asarray(p["batch"][0], np.float64), p["h"])
    assert np.abs(gp_after - aux["gp"]).max() > 1e-6 * np.abs(aux["gp"]).max()
    # both targets moved, by tau towards the NEW parameters
    assert np.allclose(new["QT"], TAU * new["Q"] + (1 - TAU) * st["QT"], rtol=0, atol=1e-15)
    assert np.allclose(new["PT"], TAU * new["P"] + (1 - TAU) * st["PT"], rtol=0, atol=1e-15)
    assert (new["q_count"], new["pi_count"]) == (1, 1)


def test_critic_loss_by_hand_with_a_terminated_row():
    q = np.array([[1.0, 2.0], [3.0, 0.5]])
    qn = np.array([[0.5, 1.5], [2.0, -1.0]])
    y, loss, dq = tw.critic_loss(q, qn, np.array([1.0, 2.0]), np.array([0.0, 1.0]), 0.5)
    assert np.array_equal(y, [1.25, 2.0])                             # row 1 is terminated: its target is the reward alone
    assert np.array_equal(dq, [[-0.125, 0.375], [0.5, -0.75]])        # 2 (q - y) / (E B), E = B = 2
    assert np.array_equal(loss, [0.3125, 1.625])                      # mean over the two critics
    y1, loss1, dq1 = tw.critic_loss(q[:, :1], qn[:, :1], np.array([1.0, 2.0]), np.array([0.0, 1.0]), 0.5)      # DDPG: one critic
    assert np.array_equal(y1, [1.25, 2.0]) and np.array_equal(dq1, [[-0.25], [1.0]]) and np.array_equal(loss1, [0.0625, 1.0])


def test_target_action_by_hand_hits_each_clip():
    """a policy with zero weights and head bias (0, 2): tanh = (0, 0.9640...) on every row; smoothing_epsilon 0.2, clip 0.5"""
    ps = nets.MLPSpec(3, [4], 2, nets.ACT_RELU, False, False)
    pt = np.zeros(ps.n_params)
    pt[ps.head["b"]:ps.head["b"] + 2] = [0.0, 2.0]
    h = dict(smoothing_epsilon=0.2, smoothing_clip_value=0.5)
    noise = np.array([[1.0, -1.0], [5.0, 5.0], [-5.0, -5.0], [0.0, 0.0]])
    a = tw.target_action(ps, pt, np.ones((4, 3)), noise, h)
    t2 = np.tanh(2.0)
    assert np.allclose(a, [[0.2, t2 - 0.2],       # inside both clips
                           [0.5, 1.0],            # noise 1.0 -> inner clip 0.5; 0.964 + 0.5 -> outer clip 1
                           [-0.5, t2 - 0.5],      # noise -1.0 -> inner clip -0.5
                           [0.0, t2]], rtol=0, atol=1e-15)
    pt[ps.head["b"]:ps.head["b"] + 2] = [0.0, -2.0]
    assert tw.target_action(ps, pt, np.ones((1, 3)), noise[2:3], h)[0, 1] == -1.0      # the lower outer clip
    assert np.array_equal(tw.target_action(ps, pt, np.ones((1, 3)), None, h), np.tanh([[0.0, -2.0]]))       # DDPG: no noise


def test_act_by_hand():
    ps = nets.MLPSpec(3, [4], 2, nets.ACT_RELU, False, False)
    pp = np.zeros(ps.n_params)
    pp[ps.head["b"]:ps.head["b"] + 2] = [0.0, 2.0]
    a, proc = tw.act(ps, pp, np.ones((2, 3)), np.array([[1.0, 1.0], [-3.0, -3.0]]), 0.1, [-2.0, 0.0], [4.0, 10.0])
    assert np.allclose(a, [[0.1, 1.0], [-0.3, np.tanh(2.0) - 0.3]], atol=1e-15)
    assert np.allclose(proc, [[-2 + 0.5 * 1.1 * 6, 10.0], [-2 + 0.5 * 0.7 * 6, 5 * (np.tanh(2.0) + 0.7)]], atol=1e-14)
    a0, _ = tw.act(ps, pp, np.ones((2, 3)), None, 0.0, [-1, -1], [1, 1])
    assert np.array_equal(a0, np.tanh([[0.0, 2.0]] * 2))


def test_an_exact_tie_gets_half_the_seed_on_each_critic():
    qa = np.array([[1.0, 1.0], [2.0, 3.0], [5.0, 4.0]])
    mn, seed = tw.policy_seed(qa)
    assert np.array_equal(mn, [1.0, 2.0, 4.0])
    assert np.array_equal(seed, [[-1 / 6, -1 / 6], [-1 / 3, 0.0], [0.0, -1 / 3]])
    import torch
    t = torch.tensor(qa, requires_grad=True)
    (-t.min(dim=1).values).mean().backward()       # (min(dim) sends a tie to ONE index; amin splits it evenly as jnp.min does)
    t2 = torch.tensor(qa, requires_grad=True)
    (-t2.amin(dim=1)).mean().backward()
    assert np.array_equal(t2.grad.numpy(), seed)


def test_targets_do_not_move_on_a_critic_only_step():
    p = _problem()
    st = p["state"]
    new, met, _ = tw.update(p["ps"], p["qs"], st, p["batch"], _noise(p), p["h"], LR, LR, TAU, do_policy_step=False)
    for k in ("QT", "PT", "P", "pm", "pv"):
        assert np.array_equal(new[k], st[k]), k
    assert not np.array_equal(new["Q"], st["Q"]) and (new["q_count"], new["pi_count"]) == (1, 0)
    assert set(met) == {"loss/q_loss", "gradients/critic_grad_norm"}
    full, fmet, _ = tw.update(p["ps"], p["qs"], st, p["batch"], _noise(p), p["h"], LR, LR, TAU)
    assert np.array_equal(full["Q"], new["Q"])                                         # the same critic step
    assert np.allclose(full["QT"], TAU * new["Q"] + (1 - TAU) * st["QT"], rtol=0, atol=1e-15)     # Polyak from the STEPPED critics
    assert np.allclose(full["PT"], TAU * full["P"] + (1 - TAU) * st["PT"], rtol=0, atol=1e-15)
    assert (full["q_count"], full["pi_count"]) == (1, 1) and set(fmet) == set(tw.METRICS)
    # the policy step reads the critics AFTER the critic step
    _, gp_before, _ = tw.policy_grads(p["ps"], p["qs"], st["P"], st["Q"], np.asarray(p["batch"][0], np.float64), p["h"])
    _, gp_after, _ = tw.policy_grads(p["ps"], p["qs"], st["P"], new["Q"], np.asarray(p["batch"][0], np.float64), p["h"])
    first = 10.0 * full["pm"]                       # a first Adam step's first moment is gradient / 10
    assert np.abs(first - gp_after).max() < 1e-12 and np.abs(first - gp_before).max() > 1e-9


@pytest.mark.parametrize("part", [True, False])
def test_key_chain_against_the_oracle(part):
    key = prng.prng_key(17)
    B, A = 9, 3
    new_key, noise = tw.smoothing_noise(key, B, A, part)
    ks = prng.split(key, B + 1, part)
    assert np.array_equal(new_key, ks[0])
    for i in (0, 1, B - 1):
        assert np.array_equal(noise[i], prng.normal(ks[1 + i], (A,), part)), i
    assert noise.shape == (B, A) and len({tuple(r) for r in noise}) == B
    # acting: ONE draw of shape (N, A) from the sub-key, not a key per row
    k2, n2 = tw.acting_noise(key, B, A, part)
    k, sub = prng.split(key, 2, part)
    assert np.array_equal(k2, k) and np.array_equal(n2, prng.normal(sub, (B, A), part))
    assert not np.array_equal(n2[0], prng.normal(prng.split(sub, B, part)[0], (A,), part))
    # the library's host split is the oracle's (the update's returned key comes from it)
    from rlx_amd.hip import lib as L
    assert np.array_equal(L.threefry_split(key, B + 1, int(part))[0], ks[0])
