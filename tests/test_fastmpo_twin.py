"""CPU: the float64 FastMPO twin (tests/fastmpo_twin.py).  The reference (rl_x/algorithms/fastmpo/flax_full_jit) needs JAX, which the
build machine does not have, so the twin is pinned three ways: hand-computed known answers; agreement with the twins that
reference-executed fixtures already pin (oracle/c51.py, tests/mpo_twin.py, oracle/fastsac.py's sampler, oracle/obs_norm.py), with
every place where the references differ stated; and the plugin's registration, the struct sizes and the library's parameter counts.

Where the references differ (stated once, used below):
  * oracle/c51.py (FastSAC): an entropy term in the reward (set to zero here), two critics (the same logits are given twice), ties of
    the clipped choice go to the second critic (`<`), FastMPO's to the first (`<=`).
  * tests/mpo_twin.py (MPO): a triangular projection -- the same linear interpolation as floor/ceil with the fix-ups; alpha_mean is
    computed from log_alpha_stddev (FastMPO: log_alpha_mean, so the two are set equal here); LayerNorm eps 1e-5 (FastMPO 1e-6: the
    comparison runs the MPO twin's own network through both); torch's clip_grad_norm_ and Adam (the optimisers are compared on
    their own, not through MPO's); softplus with torch's threshold (identical below 20).
  * oracle/fastsac.py nstep_sample (FastSAC's ring): with n_steps == 1 it returns the ring's truncations untouched; FastMPO patches
    a full ring's newest row for every n_steps (fastmpo.py:497-503).  The plugin applies that patch."""
import ctypes

import numpy as np
import pytest
import torch

import fastmpo_twin as tw
import mpo_twin
from oracle import c51 as oc51
from oracle import fastsac as ofs
from oracle.obs_norm import ObservationNormalizer

D = torch.float64


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - np.asarray(exp, np.float64)) / max(np.linalg.norm(exp), 1e-30)


# ------------------------------------------------------------------------------------------------------------- 1. known answers
def _one_hot(j, NA=5):
    p = torch.zeros(1, NA, dtype=D)
    p[0, j] = 1.0
    return p


def test_projection_known_answers():
    """support {0, 1, 2, 3, 4} (v_min 0, v_max 4, 5 atoms), discount 0 so every atom lands on the reward"""
    one, zero = torch.ones(1, dtype=D), torch.zeros(1, dtype=D)
    # a non-integer position b = 1.25: 0.75 of the mass to bin 1, 0.25 to bin 2
    proj, z = tw.project(_one_hot(3), 1.25 * one, zero, 0.0, 4.0)
    assert torch.equal(z, torch.arange(5, dtype=D))
    assert np.allclose(proj.numpy(), [[0.0, 0.75, 0.25, 0.0, 0.0]], atol=1e-15)
    # an integer b = 2 > 0: l becomes 1 with weight u - b = 0, u stays 2 with weight b - l = 1 (first fix-up)
    proj, _ = tw.project(_one_hot(0), 2.0 * one, zero, 0.0, 4.0)
    assert proj.tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0]]
    # b = 0: u becomes 1 with weight b - l = 0, l stays 0 with weight u - b = 1 (second fix-up)
    proj, _ = tw.project(_one_hot(4), zero, zero, 0.0, 4.0)
    assert proj.tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0]]
    # past the upper edge: clipped to b = 4, an integer > 0
    proj, _ = tw.project(_one_hot(2), 100.0 * one, zero, 0.0, 4.0)
    assert proj.tolist() == [[0.0, 0.0, 0.0, 0.0, 1.0]]
    # discount 0.5, reward 0.5: atoms {0..4} land on {0.5, 1, 1.5, 2, 2.5}, 0.2 each: bin 0 gets half of the first, bin 1 the
    # other half, all of the second and half of the third, bin 2 likewise, bin 3 half of the last
    proj, _ = tw.project(torch.full((1, 5), 0.2, dtype=D), 0.5 * one, 0.5 * one, 0.0, 4.0)
    assert np.allclose(proj.numpy(), [[0.1, 0.4, 0.4, 0.1, 0.0]], atol=1e-15)
    # a leading critic axis shares the tables
    both, _ = tw.project(torch.stack([_one_hot(3), _one_hot(1)]), 1.25 * one, zero, 0.0, 4.0)
    assert np.allclose(both.numpy(), [[[0.0, 0.75, 0.25, 0.0, 0.0]]] * 2, atol=1e-15)


def test_clipped_choice_known_answers_and_the_tie():
    proj = torch.tensor([[[1.0, 0.0], [0.5, 0.5], [0.2, 0.8]], [[0.0, 1.0], [0.1, 0.9], [0.8, 0.2]]], dtype=D)   # [E, B, NA]
    value = torch.tensor([[1.0, 3.0, 2.0], [2.0, 3.0, 1.0]], dtype=D)      # first smaller, a tie, second smaller
    t = tw.choose_clipped(proj, value)
    assert torch.equal(t[0], t[1])
    assert t[0].tolist() == [[1.0, 0.0], [0.5, 0.5], [0.8, 0.2]]           # the tie goes to the FIRST critic (fastmpo.py:359 `<=`)


def _small(kind="fastsac", E=2, K=3, B=6, seed=0, **over):
    O, A, NA, hid = 7, 3, 11, (64, 64, 64)
    h = dict(tw.HP, action_sampling_number=K, **over)
    LP, LQ = tw.policy_layout(kind, O, A, hid), tw.critic_layout(kind, O, A, NA, hid)
    rng = np.random.default_rng(seed)
    st = dict(p=tw.make_params(seed, LP), tp=tw.make_params(seed + 1, LP),
              q=np.concatenate([tw.make_params(seed + 2 + e, LQ, 1.0) for e in range(E)]),
              tq=np.concatenate([tw.make_params(seed + 5 + e, LQ, 1.0) for e in range(E)]), d=tw.init_duals(A, h))
    dn = (rng.random(B) < 0.3).astype(np.float64)
    batch = tuple(tw._t(x) for x in (rng.standard_normal((B, O)), rng.standard_normal((B, O)), rng.standard_normal((B, A)),
                                     rng.standard_normal(B) * 15.0, dn, dn * (rng.random(B) < 0.5), rng.integers(1, 4, B)))
    return h, LP, LQ, st, batch, rng, (O, A, NA, B, K)


def test_one_sample_makes_both_weight_softmaxes_one():
    h, LP, LQ, st, batch, rng, (O, A, NA, B, K) = _small(K=1, action_clipping=True)
    eps = tw._t(rng.standard_normal((1, 2 * B, A)) * 3.0)
    out = tw.policy_and_dual_loss(tw._t(st["p"]), tw._t(st["d"]), tw._t(st["tp"]), tw._t(st["tq"]), LP, LQ, 2, batch[0], batch[1], eps, h)
    assert torch.equal(out["weights_q"], torch.ones(1, 2 * B, dtype=D))
    assert torch.equal(out["weights"], 2.0 * torch.ones(1, 2 * B, dtype=D))     # the penalty softmax is ADDED (fastmpo.py:420)
    # logsumexp over one sample is the sample: loss_eta = eta (eps_np + mean q / eta - log 1) + pt (eps_pen + mean cost / pt)
    d = tw._t(st["d"])
    eta, pt = float(tw.softplus(d[0])) + h["float_epsilon"], float(tw.softplus(d[-1])) + h["float_epsilon"]
    sa = out["q"]
    assert sa.shape == (1, 2 * B)
    mt, sdt = tw.policy_mean_std(tw._t(st["tp"]), LP, torch.cat([batch[0], batch[1]]), h)
    a = mt + sdt * eps[0]
    cost = -torch.linalg.norm(a - a.clamp(-1.0, 1.0), dim=-1)
    want = eta * (h["epsilon_non_parametric"] + float(sa.mean()) / eta) + pt * (h["epsilon_penalty"] + float(cost.mean()) / pt)
    assert abs(float(out["loss_eta"]) - want) < 1e-9 * abs(want)


@pytest.mark.parametrize("kind", ["fastsac", "fasttd3", "mpo"])
def test_online_equal_to_target_policy_has_zero_kl_terms_and_gradients(kind):
    h, LP, LQ, st, batch, rng, (O, A, NA, B, K) = _small(kind=kind)
    p = tw._t(st["tp"]).requires_grad_(True)                  # online == target
    eps = tw._t(rng.standard_normal((K, 2 * B, A)))
    out = tw.policy_and_dual_loss(p, tw._t(st["d"]), tw._t(st["tp"]), tw._t(st["tq"]), LP, LQ, 2, batch[0], batch[1], eps, h)
    assert float(out["kl_mean"].detach().abs().max()) == 0.0 and float(out["kl_std"].detach().abs().max()) < 1e-15
    alpha = tw.softplus(tw._t(st["d"])[1:1 + 2 * A])
    kl_part = (alpha[:A] * out["kl_mean"].mean(0)).sum() + (alpha[A:] * out["kl_std"].mean(0)).sum()
    g = torch.autograd.grad(kl_part, p)[0]
    assert float(g.abs().max()) < 1e-9                         # both KL terms' policy gradients vanish (alpha ~ 1000)
    met = dict(zip(tw.POLICY_METRICS, out["metrics"]))
    assert met["kl/mean_kl_mean"] == 0.0 and abs(met["kl/mean_kl_std"]) < 1e-15 and abs(met["loss/loss_kl_std"]) < 1e-11


def test_optax_clip_below_at_and_above_the_bound():
    g = np.array([3.0, 4.0])                                                       # norm 5
    for bound, want in ((6.0, g), (5.0, g / 5.0 * 5.0), (2.5, np.array([1.5, 2.0])), (-1.0, g)):
        got, norm = tw.clip_by_global_norm(g, bound)
        assert norm == 5.0 and np.array_equal(got, want), (bound, got)
    # norm == bound takes the scaled branch (optax: `g_norm < max_norm` keeps, else scales); torch's rule would scale by c / (n + 1e-6)
    got, _ = tw.clip_by_global_norm(np.array([3.0, 4.0]), 5.0)
    assert np.array_equal(got, (np.array([3.0, 4.0]) / 5.0) * 5.0)


def test_adamw_incremental_update_and_clamps_known_answers():
    p, g = np.array([1.0, -2.0]), np.array([0.5, 0.25])
    # first step from zero moments: mhat = g, vhat = g^2 -> update g / (|g| + eps) + wd p
    p2, m2, v2 = tw.adamw(p, g, np.zeros(2), np.zeros(2), 0, 0.1, 0.9, 0.95, 0.01)
    assert np.allclose(m2, 0.1 * g) and np.allclose(v2, 0.05 * g * g)
    assert np.allclose(p2, p - 0.1 * (g / (np.abs(g) + 1e-8) + 0.01 * p), rtol=0, atol=1e-15)
    # second step: the bias corrections of count 2
    p3, m3, v3 = tw.adamw(p2, g, m2, v2, 1, 0.1, 0.9, 0.95, 0.0)
    mh, vh = (0.9 * m2 + 0.1 * g) / (1 - 0.81), (0.95 * v2 + 0.05 * g * g) / (1 - 0.9025)
    assert np.allclose(p3, p2 - 0.1 * mh / (np.sqrt(vh) + 1e-8), rtol=0, atol=1e-15)
    assert np.array_equal(tw.incremental_update(np.array([1.0]), np.array([3.0]), 0.25), [2.5])
    h = dict(tw.HP)
    d = np.array([-30.0, -20.0, 5.0, -19.0, 7.0, -40.0])           # A = 2: eta | alpha_mean | alpha_std | penalty temperature
    assert tw.clamp_duals(d, 2, h).tolist() == [-18.0, -18.0, 5.0, -18.0, 7.0, -40.0]    # the penalty temperature is not clamped


# ------------------------------------------------------------------------------------------------------------- 2. other twins
def test_critic_loss_equals_the_c51_oracle_with_one_critic_and_one_sample():
    rng = np.random.default_rng(3)
    B, NA, gamma, v_min, v_max = 9, 21, 0.97, -20.0, 20.0
    ql, tl = rng.standard_normal((B, NA)), rng.standard_normal((B, NA)) * 2.0
    r, ns = rng.standard_normal(B) * 15.0, rng.integers(1, 4, B).astype(np.float64)
    dn = (rng.random(B) < 0.3).astype(np.float64)
    tr = dn * (rng.random(B) < 0.5)
    r[0], dn[0] = 4.0, 1.0            # lands exactly on an atom (b an integer > 0); r[1]: b = 0
    r[1], dn[1], tr[1] = -20.0, 1.0, 0.0
    o = oc51.critic_loss(ql, ql, tl, tl, r, dn, tr, ns, np.zeros(B), 1.0, gamma, v_min, v_max, False)
    h = dict(tw.HP, gamma=gamma, v_min=v_min, v_max=v_max, clipped_double_q_learning=False)
    logits = tw._t(ql)[None].clone().requires_grad_(True)
    target, value = tw.target_distribution(tw._t(tl)[None, None], tw._t(r), tw._t(dn), tw._t(tr), tw._t(ns), h, 1)
    loss = tw.cross_entropy(target, logits)
    g = torch.autograd.grad(loss, logits)[0][0].numpy()
    assert _rel(target[0].numpy(), o["target1"]) < 1e-12
    assert abs(float(loss.detach()) - o["q_loss"] / 2.0) < 1e-12 * abs(o["q_loss"])      # the oracle sums two (here identical) critics
    assert _rel(g, o["d_q1"]) < 1e-12
    assert abs(float(value.min()) - o["q_min"]) < 1e-12 and abs(float(value.max()) - o["q_max"]) < 1e-12


def _as_mpo(LQm, H, in_dim, out):
    """the MPO twin's layout as a FastMPO `mpo`-kind layout: the same order of blocks"""
    L = tw.layout("mpo", in_dim, (H, H, H), out)
    assert L["n"] == LQm["n"] and all(L[a] == LQm[b] for a, b in (("W0", "W0"), ("g0", "g0"), ("be0", "be0"), ("W2", "W2"), ("Wh", "Wh")))
    return L


def test_losses_and_gradients_equal_the_mpo_twin(monkeypatch):
    """E = 1, log_alpha_mean == log_alpha_stddev elementwise, the same LayerNorm eps: the critic loss and the actor and dual losses and
    gradients equal tests/mpo_twin.py's to 1e-10.  Compared through the optimiser-free quantities the MPO twin returns (gp, gq, gd
    and the metrics); its clip_grad_norm_ + Adam are torch's, FastMPO's are optax's."""
    monkeypatch.setattr(tw, "LN_EPS", 1e-5)                    # the MPO twin's torch.nn.LayerNorm eps
    O, A, H, NA, B, S = 9, 4, 64, 21, 7, 5
    for clip in (True, False):
        hm = dict(mpo_twin.HP, action_sampling_number=S, action_clipping=clip, v_min=-30.0, v_max=30.0, policy_min_scale=0.1, max_grad_norm=-1.0)
        LPm, LQm = mpo_twin.policy_layout(O, A, H), mpo_twin.critic_layout(O, A, H, NA)
        p, q = mpo_twin.make_params(4, O, O, A, H, NA)
        tp, tq = mpo_twin.make_params(5, O, O, A, H, NA)
        rng = np.random.default_rng(6)
        d = mpo_twin.init_duals(A, hm)
        d[1 + A:1 + 2 * A] = rng.uniform(-1.0, 3.0, A)
        d[1:1 + A] = d[1 + A:1 + 2 * A]                          # log_alpha_mean == log_alpha_stddev
        d[0], d[-1] = 1.5, 0.5
        nd = 2 * A + 2
        st = dict(p=p, pm=np.zeros(p.size), pv=np.zeros(p.size), tp=tp, q=q, qm=np.zeros(q.size), qv=np.zeros(q.size), tq=tq, d=d,
                  dm=np.zeros(nd), dv=np.zeros(nd))
        dn = (rng.random(B) < 0.3).astype(np.float64)
        batch = (rng.standard_normal((B, O)), rng.standard_normal((B, O)), rng.standard_normal((B, A)), rng.standard_normal(B) * 20.0, dn,
                 dn * (rng.random(B) < 0.5), rng.integers(1, 4, B).astype(np.float64))
        eps_c, eps_a = rng.standard_normal((S, B, A)) * 2.0, rng.standard_normal((S, 2 * B, A)) * 2.0
        _, mm, ex = mpo_twin.update(st, LPm, LQm, batch, eps_c, eps_a, hm, 1)
        mm = dict(zip(mpo_twin.METRICS, mm))
        h = dict(tw.HP, action_sampling_number=S, action_clipping=clip, v_min=-30.0, v_max=30.0, policy_min_scale=0.1, gamma=hm["gamma"],
                 clipped_double_q_learning=False)
        LP, LQ = _as_mpo(LPm, H, O, 2 * A), _as_mpo(LQm, H, O + A, NA)
        bt = tuple(tw._t(x) for x in batch)
        qt = tw._t(q).requires_grad_(True)
        loss, m4, exc = tw.critic_loss(qt, tw._t(tq), tw._t(tp), LP, LQ, 1, bt, tw._t(eps_c), h)
        assert _rel(exc["target"][0].numpy(), ex["target_pmf"]) < 1e-10          # floor/ceil == triangular: one linear interpolation
        assert abs(m4[0] - mm["loss/critic_loss"]) < 1e-10 * abs(m4[0])
        assert _rel(torch.autograd.grad(loss, qt)[0].numpy(), ex["gq"]) < 1e-10
        pt_, dt_ = tw._t(p).requires_grad_(True), tw._t(d).requires_grad_(True)
        out = tw.policy_and_dual_loss(pt_, dt_, tw._t(tp), tw._t(tq), LP, LQ, 1, bt[0], bt[1], tw._t(eps_a), h)
        gp, gd = (x.numpy() for x in torch.autograd.grad(out["actor_loss"] + out["dual_loss"], (pt_, dt_)))
        fm = dict(zip(tw.POLICY_METRICS, out["metrics"]))
        assert _rel(out["q"].numpy(), ex["q"]) < 1e-10 and _rel(out["weights"].numpy(), ex["weights"]) < 1e-10
        for a, b in (("loss/actor_loss", "loss/actor_loss"), ("loss/dual_loss", "loss/dual_loss"), ("loss/loss_eta", "loss/loss_eta"),
                     ("dual/eta", "dual/eta"), ("dual/penalty_temperature", "dual/penalty_temperature"), ("kl/mean_kl_mean", "kl/mean_kl_mean"),
                     ("kl/mean_kl_std", "kl/mean_kl_std"), ("policy/std_min_mean", "policy/std_min_mean")):
            assert abs(fm[a] - mm[b]) <= 1e-10 * max(abs(mm[b]), 1.0), (a, fm[a], mm[b])
        assert abs(fm["loss/loss_alpha_mean"] + fm["loss/loss_alpha_std"] - mm["loss/loss_alpha"]) < 1e-10
        assert _rel(gp, ex["gp"]) < 1e-10
        # MPO's alpha_mean is a function of log_alpha_stddev: its gradient there is the SUM of FastMPO's two; log_alpha_mean has none
        gd_m = gd.copy()
        gd_m[1 + A:1 + 2 * A] += gd_m[1:1 + A]
        gd_m[1:1 + A] = 0.0
        assert _rel(gd_m, ex["gd"]) < 1e-10 and np.all(gd[1:1 + A] != 0.0)


@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("full", [False, True])
def test_sampler_equals_the_fastsac_ring_twin_up_to_the_stated_patch(n_steps, full):
    rng = np.random.default_rng(8)
    cap, N, O, A, U, B = 12, 5, 4, 2, 4, 9
    dn = (rng.random((cap, N)) < 0.25).astype(np.float32)
    ring = dict(states=rng.standard_normal((cap, N, O)).astype(np.float32), next_states=rng.standard_normal((cap, N, O)).astype(np.float32),
                actions=rng.standard_normal((cap, N, A)).astype(np.float32), rewards=rng.standard_normal((cap, N)).astype(np.float32),
                dones=dn, truncations=(dn * (rng.random((cap, N)) < 0.5)).astype(np.float32))
    pos, size = (7, cap) if full else (8, 8)
    ms = tw.max_start(size, cap, n_steps)
    assert ms == (cap if full else max(1, size - n_steps + 1))
    idx_t, idx_e = rng.integers(0, ms, (U, B)), rng.integers(0, N, (U, B))
    if full:
        idx_t[0, :3] = (pos - 1) % cap                       # the patched row is sampled
    got = tw.nstep_sample(ring, pos, size, cap, n_steps, 0.97, idx_t, idx_e)
    ref = ofs.nstep_sample(ring, pos, size, cap, n_steps, 0.97, idx_t.reshape(-1), idx_e.reshape(-1))
    for k, (g, r) in enumerate(zip(got, ref)):
        r = r.reshape(g.shape)
        if k == 5 and n_steps == 1 and full:
            # the one difference: FastSAC's ring returns the raw truncations for n_steps == 1; FastMPO's newest row of a full ring
            # counts as truncated unless done.  The plugin's patch, restated:
            from rlx_amd.algorithms.fastmpo.hip.fastmpo import patch_newest_truncation
            last = (pos - 1) % cap
            r = patch_newest_truncation(np, idx_t, got[4], r, last)
            assert np.any(r != ref[5].reshape(g.shape))
            rt = patch_newest_truncation(torch, torch.from_numpy(idx_t), torch.from_numpy(got[4]), torch.from_numpy(ref[5].reshape(g.shape)), last)
            assert np.array_equal(rt.numpy(), r)                     # the same function on torch tensors, as the plugin calls it
        assert np.array_equal(g, r), k


def test_normaliser_merge_equals_the_obs_norm_oracle_on_the_concatenated_rows():
    rng = np.random.default_rng(9)
    U, B, O = 4, 11, 6
    ref = ObservationNormalizer(O)
    st = dict(mean=np.zeros(O), var=np.ones(O), std=np.ones(O), count=0.0)
    for it in range(3):
        s, s2 = rng.standard_normal((U, B, O)) * (1.0 + it) + it, rng.standard_normal((U, B, O)) - it
        st = tw.normalizer_merge(st, s, s2)
        ref.update(np.concatenate([s.reshape(-1, O), s2.reshape(-1, O)]))          # ONE update of 2 U B rows (fastmpo.py:550-565)
        assert _rel(st["mean"], ref.running_mean[0]) < 1e-13 and _rel(st["var"], ref.running_var[0]) < 1e-13
        assert _rel(st["std"], ref.running_std_dev[0]) < 1e-13 and st["count"] == ref.count == 2 * U * B * (it + 1)
    # two updates (states, then next states: what fastsac.hip does) are NOT the same merge
    two = ObservationNormalizer(O)
    two.update(s.reshape(-1, O))
    two.update(s2.reshape(-1, O))
    one = ObservationNormalizer(O)
    one.update(np.concatenate([s.reshape(-1, O), s2.reshape(-1, O)]))
    assert _rel(two.running_var[0], one.running_var[0]) > 1e-6


def test_float32_step_gap_of_the_widest_case(monkeypatch):
    """Where the GPU shapes test's one wider bar comes from (tests/test_gpu_fastmpo_shapes.py, STEP_TOL): the twin's own arithmetic in
    float32 (torch autograd on the CPU, the optimiser still in float64) against the float64 twin, on the `defaults` case -- the
    reference's 768-384-192 LayerNorm critics on 8 rows, two critic steps.  The first Adam step is sign-like and hides gradient
    rounding; the second does not.  The figure is a property of the number format, not of the library."""
    import fastmpo_cases as fc
    c = fc.Case(203, "fastsac", E=2, NA=101, A=3, K=64, B=8, P=1, G=2, policy_hidden=(512, 256, 128), critic_hidden=(768, 384, 192))
    n64 = c.twin()[0]
    monkeypatch.setattr(tw, "D", torch.float32)
    n32 = c.twin()[0]
    g = n64["qm"]
    sel = np.abs(g) > 1e-3 * np.sqrt(np.mean(g * g))
    gap = _rel((n32["q"] - c.st["q"])[sel], (n64["q"] - c.st["q"])[sel])
    print("float32 step gap:", gap)
    # (5e-4 bounds the float32 run's own figure here; the GPU test's bar is stated from its GPU measurement)
    assert sel.mean() > 0.9 and gap < 5e-4 and _rel(n32["qm"], n64["qm"]) < 1e-5


# ------------------------------------------------------------------------------------------------------------- 3. library and plugin
def test_struct_sizes_and_library_param_counts():
    from rlx_amd.hip import FastMpoDesc, FastMpoHparams, fastmpo_desc
    from rlx_amd.hip import lib as L
    assert ctypes.sizeof(FastMpoDesc) == 7 * 4 + 2 * 3 * 4 and ctypes.sizeof(FastMpoHparams) == 21 * 4 + 6 * 4      # include/rlx_hip.h
    for name in ("rlx_fastmpo_param_count", "rlx_fastmpo_act_f32", "rlx_fastmpo_update_f32"):
        assert name in L.EXPORTED_SYMBOLS
    lib = L.load_library()
    O, A, NA = 48, 12, 101
    for kind in tw.KINDS:
        LP, LQ = tw.policy_layout(kind, O, A, tw.POLICY_WIDTHS[kind]), tw.critic_layout(kind, O, A, NA, tw.CRITIC_WIDTHS[kind])
        d = fastmpo_desc(O, O, A, NA, True, kind, kind)                    # the reference's widths filled in
        assert tuple(d.policy_hidden) == tw.POLICY_WIDTHS[kind] and tuple(d.critic_hidden) == tw.CRITIC_WIDTHS[kind]
        assert lib.rlx_fastmpo_param_count(ctypes.byref(d), 0) == LP["n"]
        assert lib.rlx_fastmpo_param_count(ctypes.byref(d), 1) == LQ["n"]
        assert lib.rlx_fastmpo_param_count(ctypes.byref(d), 2) == 2 * A + 2
    LQ = tw.critic_layout("fastsac", O, A, NA, (768, 384, 192))
    assert LQ["n"] == (60 * 768 + 3 * 768) + (768 * 384 + 3 * 384) + (384 * 192 + 3 * 192) + (192 * 101 + 101)
    LQ = tw.critic_layout("mpo", O, A, NA, (512, 256, 128))
    assert LQ["n"] == (60 * 512 + 3 * 512) + (512 * 256 + 256) + (256 * 128 + 128) + (128 * 101 + 101)
    mixed = fastmpo_desc(O, 40, A, NA, False, "fasttd3", "mpo", (64, 128, 192), (256, 64, 128))
    assert lib.rlx_fastmpo_param_count(ctypes.byref(mixed), 0) == tw.policy_layout("fasttd3", O, A, (64, 128, 192))["n"]
    assert lib.rlx_fastmpo_param_count(ctypes.byref(mixed), 1) == tw.critic_layout("mpo", 40, A, NA, (256, 64, 128))["n"]
    bad = fastmpo_desc(O, O, A, NA, True, 3, 0, (64, 64, 64), (64, 64, 64))
    assert lib.rlx_fastmpo_param_count(ctypes.byref(bad), 0) == -1 and lib.rlx_fastmpo_param_count(ctypes.byref(d), 3) == -1


REFERENCE_DEFAULTS = dict(
    device="gpu", nr_parallel_seeds=1, total_timesteps=2000158720, critic_network_type="fastsac", dual_critic=True,
    policy_network_type="fastsac", action_clipping=False, action_rescaling="none", policy_learning_rate=3e-4, critic_learning_rate=3e-4,
    dual_learning_rate=1e-2, anneal_policy_learning_rate=False, anneal_critic_learning_rate=False, anneal_dual_learning_rate=False,
    policy_weight_decay=0.001, critic_weight_decay=0.001, dual_weight_decay=0.0, adam_beta1=0.9, adam_beta2=0.95, max_grad_norm=40.0,
    collect_data_with_online_policy=False, action_sampling_number=4, epsilon_non_parametric=0.1, epsilon_parametric_mu=0.01,
    epsilon_parametric_sigma=1e-6, epsilon_penalty=0.001, init_log_eta=10.0, init_log_alpha_mean=10.0, init_log_alpha_stddev=1000.0,
    init_log_penalty_temperature=10.0, float_epsilon=1e-8, min_log_temperature=-18.0, min_log_alpha=-18.0, policy_init_scale=0.5,
    policy_min_scale=0.1, batch_size=8192, buffer_size_per_env=1024, learning_starts=10, v_min=-20.0, v_max=20.0, critic_tau=0.125,
    policy_tau=0.3, gamma=0.97, nr_atoms=101, n_steps=1, clipped_double_q_learning=False, nr_critic_updates_per_policy_update=4,
    nr_policy_updates_per_step=2, enable_observation_normalization=True, normalizer_epsilon=1e-8, logging_frequency=40960,
    evaluation_and_save_frequency=18350080, evaluation_active=False)      # fastmpo/flax_full_jit/default_config.py, value by value


def test_fastmpo_hip_is_registered_with_the_reference_defaults():
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.fastmpo.hip as plugin
    assert plugin.FASTMPO_HIP == "fastmpo.hip"
    cfg = am.get_algorithm_config("fastmpo.hip")
    got = {k: cfg[k] for k in cfg.keys() if k != "name"}
    assert got.pop("threefry_partitionable") is True
    assert got == REFERENCE_DEFAULTS
    for k in ("gamma", "v_min", "v_max", "critic_tau", "policy_tau", "action_sampling_number", "policy_min_scale", "adam_beta2"):
        assert tw.HP[k] == REFERENCE_DEFAULTS[k]                 # the twin's defaults are the reference's too
    model = am.get_algorithm_model_class("fastmpo.hip")
    assert model.__name__ == "FastMPO"
    props = model.general_properties()
    assert [t.name for t in props.action_space_types] == ["CONTINUOUS"]
    assert [t.name for t in props.data_interface_types] == ["TORCH"]


def _config(**alg):
    import types
    from rlx_amd.algorithms import algorithm_manager as am
    import rlx_amd.algorithms.fastmpo.hip  # noqa: F401
    cfg = am.get_algorithm_config("fastmpo.hip")
    for k, v in alg.items():
        cfg[k] = v
    sn = types.SimpleNamespace
    return sn(algorithm=cfg, runner=sn(save_model=False, track_console=False, track_tb=False, track_wandb=False),
              environment=sn(seed=0, nr_envs=8))


@pytest.mark.parametrize("flags, msg", [(dict(nr_parallel_seeds=2), "Parallel seeds"), (dict(device="cpu"), "MI355X"),
                                        (dict(clipped_double_q_learning=True, dual_critic=False), "dual_critic"),
                                        (dict(learning_starts=0), "n_steps"), (dict(action_rescaling="tanh"), "action_rescaling"),
                                        (dict(critic_network_type="simba"), "network_type")])
def test_fastmpo_hip_refuses_before_any_device_work(flags, msg, monkeypatch):
    import rlx_amd.hip.lib as L
    from rlx_amd.algorithms.fastmpo.hip.fastmpo import FastMPO

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(L.Ctx, "__init__", no_device)
    with pytest.raises(ValueError, match=msg):
        FastMPO(_config(**flags), None, None, "/nonexistent", None)
