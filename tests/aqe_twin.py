"""CPU twin (test infrastructure) of aqe.hip: the reference's AQE `update` restated in numpy, written from
rl_x/algorithms/aqe/flax/aqe.py:145-259 and critic.py.

  critic step i  aqe.py:230-240  y = r + gamma (1 - term) (mean of the K = T - nr_dropped_q_values lowest of the T = E H POOLED values
                                 of ALL target nets - alpha logp'); loss = mean over batch and all T heads of (q - y)^2; plain Adam of
                                 all E critics, Polyak; step i + 1 sees the result
  policy step    aqe.py:245-251  alpha logp - mean over ALL T heads (after the G steps) on batch 0; SAC's entropy loss
  metrics        aqe.py:242      q_loss and critic_grad_norm are the means over the G steps

The noise is an INPUT: the key chain is checked separately against oracle/prng.py.  Built on tests/tqc_twin.py (specs with H outputs
per critic, critic_forward -> [B, E H], the state layout), tests/redq_twin.py (zero_state, the shape of the loop) and oracle/sac.py
(policy, tanh-Gaussian log-prob, Polyak).  The reference's AQE exists in JAX only and JAX is not installed: PARITY UNPINNED by the
reference; tests/test_aqe_twin.py pins the twin with hand-computed answers and float64 torch.autograd.

Q matrices here are [B, T], column i = e H + h (`reshape(nr_total_q_values)` per sample); the library's are [E, B, H].  The dtype of
the state is the dtype of the whole evaluation: float64 for the reference values, float32 to measure what float32 arithmetic
itself costs (tests/test_gpu_aqe.py, tests/test_gpu_aqe_loss.py).
"""
import numpy as np

import redq_twin as rt
import tqc_twin as tt
from oracle import nets, sac

METRICS = tt.METRICS
STATE_KEYS = tt.STATE_KEYS
zero_state = rt.zero_state


def make_specs(policy_obs_dim, critic_obs_dim, act_dim, policy_hidden, critic_hidden, H):
    return tt.make_specs(policy_obs_dim, critic_obs_dim, act_dim, policy_hidden, critic_hidden, H)


def problem(seed, O, A, B, ph, qh, E, H, dropped, G, Oc=None):
    """tests/redq_twin.py's input recipe (float32 values: lecun init + 0.02 noise, policy head scale 0.1, targets = online + 0.01
    noise, log_alpha = -0.3) for G batches -> dict(ps, qs, state, batch, cbatch or None, h)"""
    rng = np.random.default_rng(seed)
    ps, qs = make_specs(O, O if Oc is None else Oc, A, ph, qh, H)
    pp = (sac.lecun_normal_init(ps, rng) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    pp[ps.head["W"]:ps.head["W"] + ps.head["in"] * ps.head["out"]] *= 0.1
    qp = (np.concatenate([sac.lecun_normal_init(qs, rng) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params)).astype(np.float32)
    qtp = (qp + 0.01 * rng.standard_normal(qp.shape)).astype(np.float32)
    f = lambda x: x.astype(np.float32)
    batch = (f(rng.standard_normal((G, B, O))), f(rng.standard_normal((G, B, O))), f(np.tanh(rng.standard_normal((G, B, A)))),
             f(rng.standard_normal((G, B))), f(rng.random((G, B)) < 0.2))
    cbatch = None if Oc is None else (f(rng.standard_normal((G, B, Oc))), f(rng.standard_normal((G, B, Oc))))
    h = dict(gamma=0.99, target_entropy=-float(A), ensemble_size=E, nr_heads_per_net=H, nr_dropped_q_values=dropped, q_update_steps=G,
             log_std_min=-20.0, log_std_max=2.0)
    return dict(ps=ps, qs=qs, state=zero_state(pp, qp, qtp, np.float32(-0.3)), batch=batch, cbatch=cbatch, h=h)


def truncated_mean_target(q_next, K):
    """aqe.py:165 for a batch: q_next [B, T] pooled over all nets -> mean of each row's K lowest values [B]"""
    return np.sort(q_next, axis=1)[:, :K].mean(axis=1)


def critic_loss(q, q_next, rewards, terminations, alpha, next_logp, gamma, K):
    """aqe.py:164-171 for a batch: q, q_next [B, T] -> (y [B], per-sample loss [B], d mean(loss) / d q [B, T])"""
    B, T = q.shape
    y = rewards + gamma * (1 - terminations) * (truncated_mean_target(q_next, K) - alpha * next_logp)
    d = q - y[:, None]
    return y, (d * d).mean(axis=1), 2.0 * d / (B * T)


def policy_seed(qa):
    """aqe.py:197-200: qa [B, T] -> (mean_q [B], d mean_b(-mean_q) / d qa [B, T] = -1 / (B T) everywhere)"""
    B, T = qa.shape
    return qa.mean(axis=1), np.full((B, T), -1.0 / (B * T), dtype=qa.dtype)


def _K(h):
    return int(h["ensemble_size"]) * int(h["nr_heads_per_net"]) - int(h["nr_dropped_q_values"])


def critic_step(ps, qs, pp, qp, qtp, log_alpha, batch, eps1, h, cs=None, cs2=None):
    """critic_loss_fn meaned (aqe.py:149-178, :219-224) -> (q_loss, gcritic [E n], y [B]); batch = (s, s', a, r, term) of ONE step"""
    s, s2, a, r, term = batch
    cs = s if cs is None else cs
    cs2 = s2 if cs2 is None else cs2
    dt = qp.dtype
    E, H, n = int(h["ensemble_size"]), int(h["nr_heads_per_net"]), qs.n_params
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    nm, nls, _, _ = sac.policy_forward(ps, pp, s2, lo, hi)
    na, nlogp = sac.tanh_gaussian(nm, nls, eps1)
    qn, _ = tt.critic_forward(qs, qtp, E, cs2, na)
    q, caches = tt.critic_forward(qs, qp, E, cs, a)
    y, loss, dq = critic_loss(q, qn, r, term, alpha, nlogp, dt.type(h["gamma"]), _K(h))
    g = np.concatenate([nets.backward(qs, qp[e * n:(e + 1) * n], caches[e], dq[:, e * H:(e + 1) * H].astype(dt)) for e in range(E)])
    return loss.mean(), g, y


def policy_step(ps, qs, pp, qp, log_alpha, s, eps2, h, cs=None):
    """policy_entropy_loss_fn meaned (aqe.py:181-217) -> (metrics, gpolicy, g_log_alpha)"""
    cs = s if cs is None else cs
    dt = pp.dtype
    B = s.shape[0]
    E, H, n = int(h["ensemble_size"]), int(h["nr_heads_per_net"]), qs.n_params
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    cm, cls, cls_raw, pc = sac.policy_forward(ps, pp, s, lo, hi)
    std = np.exp(cls)
    ca, clogp = sac.tanh_gaussian(cm, cls, eps2)
    entropy = -clogp
    qa, caches = tt.critic_forward(qs, qp, E, cs, ca)
    mean_q, seed = policy_seed(qa)
    Oc = cs.shape[1]
    dq_da = np.zeros_like(ca)
    for e in range(E):
        _, dx = nets.backward(qs, qp[e * n:(e + 1) * n], caches[e], seed[:, e * H:(e + 1) * H].astype(dt), need_dx=True)
        dq_da += dx[:, Oc:]
    one_m = 1.0 - ca ** 2
    d_u = (alpha / B * 2.0 * ca / (one_m + 1e-6) + dq_da) * one_m     # alpha logp through a = tanh(u), as oracle/sac.py
    inside = (cls_raw > lo) & (cls_raw < hi)
    d_ls = np.where(inside, d_u * std * eps2 - alpha / B, 0.0)
    gpolicy = nets.backward(ps, pp, pc, np.concatenate([d_u, d_ls], axis=1).astype(dt))
    ga = alpha * (entropy - h["target_entropy"]).mean()
    metrics = {"loss/policy_loss": (alpha * clogp - mean_q).mean(), "loss/entropy_loss": (alpha * (entropy - h["target_entropy"])).mean(),
               "entropy/entropy": entropy.mean(), "entropy/alpha": alpha, "q_value/q_value": mean_q.mean()}
    return metrics, gpolicy, dt.type(ga)


def update(ps, qs, st, batch, eps1, eps2, h, *rates_and_critic_states):
    """`update` (aqe.py:145-259): tests/redq_twin.py's run_update over this file's steps"""
    return rt.run_update(lambda i, P, Q, QT, la, b, e1, cs, cs2: critic_step(ps, qs, P, Q, QT, la, b, e1, h, cs, cs2),
                         lambda P, Q, la, s, e2, cs: policy_step(ps, qs, P, Q, la, s, e2, h, cs),
                         st, batch, eps1, eps2, h, *rates_and_critic_states)


def losses_torch(ps, pp, qs, qp, qtp, log_alpha, batch, eps1, eps2, h, critic_states=None, critic_next_states=None):
    """ONE critic step's loss and the policy / entropy loss on the same parameters, restated with torch ops (float64) and
    differentiated by torch.autograd; the target is sort(dim=1).values[:, :K].mean(1).
    -> (q_loss, gQ, policy_loss + entropy_loss, gP, gLA)"""
    import torch
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    P, Q, LA = t(pp).requires_grad_(True), t(qp).requires_grad_(True), t(log_alpha).requires_grad_(True)
    QT = t(qtp)
    A = ps.out_dim // 2
    E, n, K = int(h["ensemble_size"]), qs.n_params, _K(h)
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    s, s2, a, r, term = (t(x) for x in batch)
    cs = s if critic_states is None else t(critic_states)
    cs2 = s2 if critic_next_states is None else t(critic_next_states)

    def pol(params, x):
        out = nets.torch_forward(ps, params, x)
        return out[:, :A], torch.clamp(out[:, A:], lo, hi)

    def qvals(params, obs, act):
        x = torch.cat([obs, act], dim=1)
        return torch.cat([nets.torch_forward(qs, params[e * n:(e + 1) * n], x) for e in range(E)], dim=1)

    def tg(mean, ls, eps):
        u = mean + torch.exp(ls) * eps
        act = torch.tanh(u)
        return act, (-0.5 * ((u - mean) / torch.exp(ls)) ** 2 - 0.5 * tt.LOG_2PI - ls - torch.log(1.0 - act ** 2 + 1e-6)).sum(1)

    alpha_g = torch.exp(LA)
    alpha = alpha_g.detach()
    na, nlp = tg(*pol(P.detach(), s2), t(eps1))
    y = r + h["gamma"] * (1 - term) * (qvals(QT, cs2, na).sort(dim=1).values[:, :K].mean(1) - alpha * nlp)
    q_loss = ((qvals(Q, cs, a) - y[:, None]) ** 2).mean()
    gQ, = torch.autograd.grad(q_loss, Q)
    ca, clp = tg(*pol(P, s), t(eps2))
    entropy = (-clp).detach()
    mean_q = qvals(Q.detach(), cs, ca).mean(dim=1)
    pe_loss = (alpha * clp - mean_q + alpha_g * (entropy - h["target_entropy"])).mean()
    gP, gLA = torch.autograd.grad(pe_loss, (P, LA))
    return q_loss.item(), gQ.numpy(), pe_loss.item(), gP.numpy(), gLA.item()
