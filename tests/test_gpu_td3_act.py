"""GPU: rlx_td3_act_f32 -- get_action (td3.py:107-112) and get_deterministic_action (:203-205) -- against tests/td3_twin.py's act on
the oracle's shape-wide normal draw (oracle/prng.py).

Tolerance: the action is tanh of a float32 chain of three products with K <= 64 and operands of order one, each off by at most
K 2^-24 ~ 4e-6 in the worst case and far less on average, plus a normal draw that agrees with the oracle's to a few float32 ulps times
epsilon = 0.1: 1e-5 absolute on the action, and that times the largest (high - low) / 2 = 5 on the processed action."""
import numpy as np
import pytest
import torch

import td3_twin as tw
from oracle import nets, prng
from rlx_amd.hip import mlp_desc

pytestmark = pytest.mark.gpu

N, O, A, HID = 37, 11, 3, [64, 64]
KEY = prng.prng_key(23)
LOW, HIGH = np.array([-2.0, 0.0, 1.0], np.float32), np.array([4.0, 10.0, 1.5], np.float32)      # asymmetric bounds
TOL = 1e-5


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


@pytest.fixture(scope="module")
def prob():
    p = tw.problem(31, O, A, N, HID, HID)
    return p["ps"], np.asarray(p["state"]["P"], np.float32), p["batch"][0]


def _act(ctx, dev, pp, obs, key, epsilon, scheme=1, inject=None):
    pd = mlp_desc(O, HID, A, nets.ACT_RELU, False, False)
    action, proc = torch.full((N, A), 9.0, device=dev), torch.full((N, A), 9.0, device=dev)
    eps = None if inject is None else _t(inject, dev)
    if eps is not None:
        ctx.dbg_set_sac_noise(eps, None)
    try:
        new_key = ctx.td3_act(pd, _t(pp, dev), _t(obs, dev), key, action, proc, _t(LOW, dev), _t(HIGH, dev), epsilon, scheme)
    finally:
        ctx.dbg_set_sac_noise(None, None)
    torch.cuda.synchronize()
    return new_key, action.cpu().numpy(), proc.cpu().numpy()


@pytest.mark.parametrize("scheme", [1, 0])
def test_act_matches_twin_on_the_oracle_draw(ctx, dev, prob, scheme):
    ps, pp, obs = prob
    key_e, noise = tw.acting_noise(KEY, N, A, bool(scheme))
    assert np.array_equal(noise, prng.normal(prng.split(KEY, 2, bool(scheme))[1], (N, A), bool(scheme)))      # ONE draw of shape (N, A)
    a_e, p_e = tw.act(ps, pp.astype(np.float64), obs, noise, 0.1, LOW, HIGH)
    key, a, p = _act(ctx, dev, pp, obs, KEY, 0.1, scheme)
    assert np.array_equal(key, key_e)
    print(f"td3 act scheme={scheme}: action {np.abs(a - a_e).max():.2e} processed {np.abs(p - p_e).max():.2e}")
    assert np.abs(a - a_e).max() <= TOL and np.abs(p - p_e).max() <= 5 * TOL
    # the injected draw: the same action, the same key
    key_i, a_i, p_i = _act(ctx, dev, pp, obs, KEY, 0.1, scheme, inject=noise)
    assert np.array_equal(key_i, key_e) and np.abs(a_i - a_e).max() <= TOL and np.abs(a_i - a).max() <= 1e-6
    # a key per row (the update's scheme) would be another action
    rows = np.stack([prng.normal(k, (A,), bool(scheme)) for k in prng.split(prng.split(KEY, 2, bool(scheme))[1], N, bool(scheme))])
    assert np.abs(tw.act(ps, pp.astype(np.float64), obs, rows, 0.1, LOW, HIGH)[0] - a).max() > 100 * TOL


def test_the_clip_is_reached_and_the_bounds_are_asymmetric(ctx, dev, prob):
    ps, pp, obs = prob
    sat = pp.copy()
    sat[ps.head["b"]:ps.head["b"] + A] = [9.0, -9.0, 0.0]               # tanh saturates: column 0 at +1, column 1 at -1
    noise = np.abs(np.random.default_rng(2).standard_normal((N, A))).astype(np.float32) * np.array([1.0, -1.0, 1.0], np.float32)
    a_e, p_e = tw.act(ps, sat.astype(np.float64), obs, noise, 0.1, LOW, HIGH)
    _, a, p = _act(ctx, dev, sat, obs, KEY, 0.1, inject=noise)
    assert np.all(a[:, 0] == 1.0) and np.all(a[:, 1] == -1.0) and np.all(np.abs(a) <= 1.0)
    assert np.all(p[:, 0] == HIGH[0]) and np.all(p[:, 1] == LOW[1])
    assert np.abs(a - a_e).max() <= TOL and np.abs(p - p_e).max() <= 5 * TOL
    assert np.all((p[:, 2] >= LOW[2]) & (p[:, 2] <= HIGH[2])) and p[:, 2].std() > 0


def test_epsilon_zero_is_deterministic_and_leaves_the_key_alone(ctx, dev, prob):
    ps, pp, obs = prob
    a_e, p_e = tw.act(ps, pp.astype(np.float64), obs, None, 0.0, LOW, HIGH)
    key, a, p = _act(ctx, dev, pp, obs, KEY, 0.0)
    assert np.array_equal(key, KEY)
    assert np.abs(a - a_e).max() <= TOL and np.abs(p - p_e).max() <= 5 * TOL
    key2, a2, p2 = _act(ctx, dev, pp, obs, prng.prng_key(99), 0.0, inject=np.ones((N, A), np.float32))      # neither key nor hook is read
    assert np.array_equal(a2, a) and np.array_equal(p2, p)
