"""CPU twin (test infrastructure) of tqc.hip: the reference's TQC `loss_fn` and `update` restated in numpy, written from
rl_x/algorithms/tqc/flax/tqc.py:139-230 and critic.py:17-55.

  target       tqc.py:155-158  sort the POOLED nr_total_atoms next-state atoms of the target nets, keep the first nr_target_atoms
  critic loss  tqc.py:161-170  quantile Huber loss over all (online atom i, target k) pairs, tau_i = (i + 0.5) / T
  policy loss  tqc.py:173-185  alpha logp - mean over all atoms of the frozen critics on (s, a_pi)
  entropy loss tqc.py:188
  update       tqc.py:211-228  per-sample keys, three plain optax.adam steps, Polyak

What is shared with SAC comes from oracle/sac.py (policy_forward, tanh_gaussian, sample_noise, polyak) and oracle/nets.py: the
policy file and the key schedule are sac/flax's.  The reference's TQC exists in JAX only and JAX is not installed: the sort /
quantile-loss part is PARITY UNPINNED by the reference; tests/test_tqc_twin.py pins it with hand-computed answers and the three
gradients with float64 torch.autograd.

FLAT LAYOUT: policy as oracle/sac.py; critics: E = ensemble_size MLPs (in_dim = Oc + A, out_dim = N = nr_atoms_per_net) back to
back.  Atom matrices are [B, T], column i = e N + n (`q_atoms.reshape(nr_total_atoms)` per sample).
"""
import numpy as np

from oracle import nets, ppo as oppo, sac

LOG_2PI = sac.LOG_2PI
METRICS = ["loss/q_loss", "loss/policy_loss", "loss/entropy_loss", "entropy/entropy", "entropy/alpha", "q_value/q_value"]


def make_specs(policy_obs_dim, critic_obs_dim, act_dim, policy_hidden, critic_hidden, nr_atoms_per_net):
    """tqc/flax/policy.py:22-41 (= sac's), critic.py:17-55 (Dense + ReLU per hidden layer, Dense(nr_atoms_per_net))"""
    ps = nets.MLPSpec(policy_obs_dim, policy_hidden, 2 * act_dim, nets.ACT_RELU, False, False)
    qs = nets.MLPSpec(critic_obs_dim + act_dim, critic_hidden, nr_atoms_per_net, nets.ACT_RELU, False, False)
    return ps, qs


def critic_forward(qs, qp, E, obs, act):
    """-> atoms [B, E N] (column e N + n), the E caches"""
    n = qs.n_params
    x = np.concatenate([obs, act], axis=1)
    outs, caches = zip(*(nets.forward(qs, qp[e * n:(e + 1) * n], x) for e in range(E)))
    return np.concatenate(outs, axis=1), caches


def truncated_target(next_atoms, rewards, terminations, alpha, next_logp, gamma, K):
    """tqc.py:156-158: y [B, K] from the pooled next-state atoms [B, T]"""
    z = np.sort(next_atoms, axis=1)[:, :K]
    return rewards[:, None] + gamma * (1 - terminations)[:, None] * (z - alpha * next_logp[:, None])


PAIR_ROWS = 4096


def pair_loss(q_atoms, y, kappa, batch=None):
    """tqc.py:161-170 for a batch: q_atoms [B, T], y [B, K] -> (per-sample loss [B], d mean_b(loss) / d q_atoms [B, T]); batch: the
    size of the batch the mean is taken over when the rows are a part of it"""
    B, T = q_atoms.shape
    K = y.shape[1]
    if B > PAIR_ROWS:                 # rows are independent: the same arithmetic per row, PAIR_ROWS of them at a time ([B, T, K] temporaries)
        parts = [pair_loss(q_atoms[i:i + PAIR_ROWS], y[i:i + PAIR_ROWS], kappa, batch=batch or B) for i in range(0, B, PAIR_ROWS)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    B = batch or B
    tau = ((np.arange(T, dtype=q_atoms.dtype) + 0.5) / T)[None, :, None]
    delta = y[:, None, :] - q_atoms[:, :, None]                       # [B, T, K]
    ad = np.abs(delta)
    huber = np.where(ad <= kappa, 0.5 * delta ** 2, kappa * (ad - 0.5 * kappa))
    w = np.abs(tau - (delta < 0))
    loss = (w * huber / kappa).mean(axis=(1, 2))
    dq = -(w * np.clip(delta, -kappa, kappa) / kappa).sum(axis=2) / (B * T * K)
    return loss, dq


def loss_and_grads(ps, pp, qs, qp, qtp, log_alpha, states, next_states, actions, rewards, terminations, eps1, eps2, h,
                   critic_states=None, critic_next_states=None, relu_toggle=()):
    """loss_fn (tqc.py:139-203) meaned over the batch (:206-209) with a hand-written reverse pass.
    h: gamma, target_entropy, ensemble_size, nr_atoms_per_net, nr_dropped_atoms_per_net, huber_kappa, log_std_min, log_std_max.
    relu_toggle: (path, layer, row, unit) entries whose ReLU on / off state is inverted in the REVERSE pass only, as in
    oracle.sac.loss_and_grads -- path "q<e>" (critic e on the replayed action), "qa<e>" (critic e on the policy's action), "pi" (the
    policy on `states`): what a float32 evaluation may legitimately return for a unit within rounding of its kink.
    -> (metrics, gpolicy, gcritic, g_log_alpha, aux) with aux = {y, q_atoms, next_atoms, next_logp, dq}."""
    cs = states if critic_states is None else critic_states
    cs2 = next_states if critic_next_states is None else critic_next_states
    dt = pp.dtype
    B = states.shape[0]
    E, N = int(h["ensemble_size"]), int(h["nr_atoms_per_net"])
    T = E * N
    K = T - E * int(h["nr_dropped_atoms_per_net"])
    kappa, gamma = dt.type(h["huber_kappa"]), dt.type(h["gamma"])
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    n = qs.n_params
    # ---- critic loss
    nm, nls, _, _ = sac.policy_forward(ps, pp, next_states, lo, hi)
    na, nlogp = sac.tanh_gaussian(nm, nls, eps1)
    next_atoms, _ = critic_forward(qs, qtp, E, cs2, na)
    y = truncated_target(next_atoms, rewards, terminations, alpha, nlogp, gamma, K)
    q_atoms, caches = critic_forward(qs, qp, E, cs, actions)
    q_loss, dq = pair_loss(q_atoms, y, kappa)
    gcritic = np.zeros(E * n, dtype=dt)

    def toggle(cache, path):
        for pth, layer, row, unit in relu_toggle:
            if pth == path:
                hh = cache["h"][layer] = cache["h"][layer].copy()
                hh[row, unit] = 0.0 if hh[row, unit] > 0 else np.finfo(hh.dtype).tiny     # the mask is (h > 0), nets._act_grad_from_out
    for e in range(E):
        toggle(caches[e], "q%d" % e)
        gcritic[e * n:(e + 1) * n] = nets.backward(qs, qp[e * n:(e + 1) * n], caches[e], dq[:, e * N:(e + 1) * N].astype(dt))
    # ---- policy loss
    cm, cls, cls_raw, pc = sac.policy_forward(ps, pp, states, lo, hi)
    std = np.exp(cls)
    ca, clogp = sac.tanh_gaussian(cm, cls, eps2)
    entropy = -clogp
    pi_atoms, pcaches = critic_forward(qs, qp, E, cs, ca)
    mean_q = pi_atoms.mean(axis=1)
    policy_loss = alpha * clogp - mean_q
    Oc = cs.shape[1]
    dq_da = np.zeros_like(ca)
    seed = np.full((B, N), -1.0 / (B * T), dtype=dt)                  # d mean_b(-mean atoms) / d atom
    toggle(pc, "pi")
    for e in range(E):
        toggle(pcaches[e], "qa%d" % e)
        _, dx = nets.backward(qs, qp[e * n:(e + 1) * n], pcaches[e], seed, need_dx=True)
        dq_da += dx[:, Oc:]
    one_m = 1.0 - ca ** 2
    d_u = (alpha / B * 2.0 * ca / (one_m + 1e-6) + dq_da) * one_m     # alpha logp through a = tanh(u), as oracle/sac.py
    inside = (cls_raw > lo) & (cls_raw < hi)
    d_ls = np.where(inside, d_u * std * eps2 - alpha / B, 0.0)
    gpolicy = nets.backward(ps, pp, pc, np.concatenate([d_u, d_ls], axis=1).astype(dt))
    # ---- entropy coefficient (tqc.py:188)
    entropy_loss = alpha * (entropy - h["target_entropy"])
    g_log_alpha = alpha * (entropy - h["target_entropy"]).mean()
    metrics = {"loss/q_loss": q_loss.mean(), "loss/policy_loss": policy_loss.mean(), "loss/entropy_loss": entropy_loss.mean(),
               "entropy/entropy": entropy.mean(), "entropy/alpha": alpha, "q_value/q_value": mean_q.mean()}
    aux = {"y": y, "q_atoms": q_atoms, "next_atoms": next_atoms, "next_logp": nlogp, "dq": dq}
    return metrics, gpolicy, gcritic, dt.type(g_log_alpha), aux


def kink_entries(spec, params, x, tau):
    """(layer, row, unit, |z| / rms) of every ReLU pre-activation of the batch within tau of zero, relative to the row's RMS
    pre-activation (float64): within float32 rounding of its kink a unit's float32 gradient may land on either side"""
    h, out = np.asarray(x, np.float64), []
    for li, L in enumerate(spec.layers):
        z = h @ params[L["W"]:L["W"] + L["in"] * L["out"]].reshape(L["in"], L["out"]) + params[L["b"]:L["b"] + L["out"]]
        m = np.abs(z) / np.sqrt((z * z).mean(axis=1, keepdims=True))
        out += [(li, int(i), int(j), float(m[i, j])) for i, j in zip(*np.nonzero(m < tau))]
        h = np.maximum(z, 0.0)
    return out


def critic_kink_delta(qs, qp_e, x_row, dq_row, layer, unit):
    """what one critic's gradient changes by when the ReLU of `unit` in `layer` is inverted in the reverse pass for ONE sample
    (x_row [1, in], dq_row [1, N]: that sample's input and seed): samples contribute independently, so the deltas of several add"""
    _, cache = nets.forward(qs, qp_e, x_row)
    g0 = nets.backward(qs, qp_e, cache, dq_row)
    hh = cache["h"][layer] = cache["h"][layer].copy()
    hh[0, unit] = 0.0 if hh[0, unit] > 0 else np.finfo(hh.dtype).tiny
    return nets.backward(qs, qp_e, cache, dq_row) - g0


STATE_KEYS = ("P", "pm", "pv", "Q", "qm", "qv", "QT", "la", "am", "av")


def zero_state(pp, qp, qtp, log_alpha):
    f = lambda x: np.asarray(x, np.float64)
    z = np.zeros_like
    return {"P": f(pp), "pm": z(f(pp)), "pv": z(f(pp)), "Q": f(qp), "qm": z(f(qp)), "qv": z(f(qp)), "QT": f(qtp),
            "la": np.array([log_alpha], np.float64), "am": np.zeros(1), "av": np.zeros(1), "count": 0}


def update(ps, qs, st, batch, eps1, eps2, h, lr, tau, critic_states=None, critic_next_states=None):
    """`update` (tqc.py:211-228) from the state st (STATE_KEYS + count): three optax.adam steps, Polyak.
    -> (new state, metrics incl. the three gradient norms, gradients (gp, gq, ga), loss_and_grads' aux)"""
    dt = st["P"].dtype
    s, s2, a, r, term = (np.asarray(x, dt) for x in batch)
    cast = lambda x: None if x is None else np.asarray(x, dt)
    met, gp, gq, ga, aux = loss_and_grads(ps, st["P"], qs, st["Q"], st["QT"], st["la"][0], s, s2, a, r, term, np.asarray(eps1, dt),
                                        np.asarray(eps2, dt), h, cast(critic_states), cast(critic_next_states))
    new = {"count": st["count"] + 1}
    new["P"], new["pm"], new["pv"] = oppo.adam_step(st["P"], gp, st["pm"], st["pv"], st["count"], lr)
    new["Q"], new["qm"], new["qv"] = oppo.adam_step(st["Q"], gq, st["qm"], st["qv"], st["count"], lr)
    new["la"], new["am"], new["av"] = oppo.adam_step(st["la"], np.array([ga], dt), st["am"], st["av"], st["count"], lr)
    new["QT"] = sac.polyak(new["Q"], st["QT"], dt.type(tau))
    met = dict(met)
    met.update({"gradients/policy_grad_norm": np.linalg.norm(gp), "gradients/critic_grad_norm": np.linalg.norm(gq),
                "gradients/entropy_grad_norm": abs(float(ga))})
    return new, met, (gp, gq, ga), aux


def loss_torch(ps, pp, qs, qp, qtp, log_alpha, states, next_states, actions, rewards, terminations, eps1, eps2, h,
               critic_states=None, critic_next_states=None):
    """The same loss restated with torch ops (float64), differentiated by torch.autograd -> (loss, gP, gQ, gLA)."""
    import torch
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    P, Q, LA = t(pp).requires_grad_(True), t(qp).requires_grad_(True), t(log_alpha).requires_grad_(True)
    QT = t(qtp)
    A = ps.out_dim // 2
    n = qs.n_params
    E, N = int(h["ensemble_size"]), int(h["nr_atoms_per_net"])
    T = E * N
    K = T - E * int(h["nr_dropped_atoms_per_net"])
    kappa = float(h["huber_kappa"])
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)

    def pol(params, x):
        out = nets.torch_forward(ps, params, x)
        return out[:, :A], torch.clamp(out[:, A:], lo, hi)

    def atoms(params, s, a):
        x = torch.cat([s, a], dim=1)
        return torch.cat([nets.torch_forward(qs, params[e * n:(e + 1) * n], x) for e in range(E)], dim=1)

    def tg(mean, ls, eps):
        u = mean + torch.exp(ls) * eps
        a = torch.tanh(u)
        return a, (-0.5 * ((u - mean) / torch.exp(ls)) ** 2 - 0.5 * LOG_2PI - ls - torch.log(1.0 - a ** 2 + 1e-6)).sum(1)

    s, s2 = t(states), t(next_states)
    cs = s if critic_states is None else t(critic_states)
    cs2 = s2 if critic_next_states is None else t(critic_next_states)
    na, nlp = tg(*pol(P.detach(), s2), t(eps1))
    alpha_g = torch.exp(LA)
    alpha = alpha_g.detach()
    z = torch.sort(atoms(QT, cs2, na), dim=1).values[:, :K]
    y = (t(rewards)[:, None] + h["gamma"] * (1 - t(terminations))[:, None] * (z - alpha * nlp[:, None]))[:, None, :]
    q = atoms(Q, cs, t(actions))[:, :, None]
    tau = ((torch.arange(T, dtype=torch.float64) + 0.5) / T)[None, :, None]
    delta = y - q
    ad = delta.abs()
    huber = torch.where(ad <= kappa, 0.5 * delta ** 2, kappa * (ad - 0.5 * kappa))
    q_loss = ((tau - (delta < 0).double()).abs() * huber / kappa).mean(dim=(1, 2))
    ca, clp = tg(*pol(P, s), t(eps2))
    entropy = (-clp).detach()
    mean_q = atoms(Q.detach(), cs, ca).mean(dim=1)
    loss = (q_loss + alpha * clp - mean_q + alpha_g * (entropy - h["target_entropy"])).mean()
    loss.backward()
    return loss.item(), P.grad.numpy(), Q.grad.numpy(), LA.grad.item()
