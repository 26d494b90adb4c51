"""CPU twin (test infrastructure) of redq.hip: the reference's REDQ `update` restated in numpy, written from
rl_x/algorithms/redq/flax/redq.py:144-261 and critic.py:17-53.

  critic step i  redq.py:228-242  y = r + gamma (1 - term) (min over the M SELECTED targets - alpha logp'); loss = mean over batch
                                  and ensemble of (q_e - y)^2; plain Adam of all E critics, Polyak; step i + 1 sees the result
  policy step    redq.py:246-253  alpha logp - min over ALL E critics (after the G steps) on batch 0; SAC's entropy loss
  metrics        redq.py:244      q_loss and critic_grad_norm are the means over the G steps

The subsets (redq.py:232-233) and the noise are INPUTS: the key chain and the shuffle are checked separately against oracle/prng.py.
Built on tests/tqc_twin.py (specs with one output per critic, critic_forward, the state layout) and oracle/sac.py (policy,
tanh-Gaussian log-prob, Polyak).  The reference's REDQ exists in JAX only and JAX is not installed: PARITY UNPINNED by the reference;
tests/test_redq_twin.py pins the twin with hand-computed answers and float64 torch.autograd.

Q matrices here are [B, E] (column e = critic e); the library's are [E, B].  The dtype of the state is the dtype of the whole
evaluation: float64 for the reference values, float32 to measure what float32 arithmetic itself costs (tests/test_gpu_redq.py).
"""
import numpy as np

import tqc_twin as tt
from oracle import nets, ppo as oppo, sac

METRICS = tt.METRICS
STATE_KEYS = tt.STATE_KEYS


def make_specs(policy_obs_dim, critic_obs_dim, act_dim, policy_hidden, critic_hidden):
    return tt.make_specs(policy_obs_dim, critic_obs_dim, act_dim, policy_hidden, critic_hidden, 1)


def zero_state(pp, qp, qtp, log_alpha, dtype=np.float64):
    st = tt.zero_state(pp, qp, qtp, log_alpha)
    del st["count"]
    st = {k: v.astype(dtype) for k, v in st.items()}
    st.update(q_count=0, pi_count=0)
    return st


def problem(seed, O, A, B, ph, qh, E, M, G, Oc=None):
    """tests/test_gpu_tqc.py's input recipe (float32 values: lecun init + 0.02 noise, policy head scale 0.1, targets = online +
    0.01 noise, log_alpha = -0.3) for G batches -> dict(ps, qs, state (float64), batch, cbatch or None, h)"""
    rng = np.random.default_rng(seed)
    ps, qs = make_specs(O, O if Oc is None else Oc, A, ph, qh)
    pp = (sac.lecun_normal_init(ps, rng) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    pp[ps.head["W"]:ps.head["W"] + ps.head["in"] * ps.head["out"]] *= 0.1
    qp = (np.concatenate([sac.lecun_normal_init(qs, rng) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params)).astype(np.float32)
    qtp = (qp + 0.01 * rng.standard_normal(qp.shape)).astype(np.float32)
    f = lambda x: x.astype(np.float32)
    batch = (f(rng.standard_normal((G, B, O))), f(rng.standard_normal((G, B, O))), f(np.tanh(rng.standard_normal((G, B, A)))),
             f(rng.standard_normal((G, B))), f(rng.random((G, B)) < 0.2))
    cbatch = None if Oc is None else (f(rng.standard_normal((G, B, Oc))), f(rng.standard_normal((G, B, Oc))))
    h = dict(gamma=0.99, target_entropy=-float(A), ensemble_size=E, in_target_minimization_size=M, q_update_steps=G, log_std_min=-20.0,
             log_std_max=2.0)
    return dict(ps=ps, qs=qs, state=zero_state(pp, qp, qtp, np.float32(-0.3)), batch=batch, cbatch=cbatch, h=h)


def critic_loss(q, q_next_sel, rewards, terminations, alpha, next_logp, gamma):
    """redq.py:163-169 for a batch: q [B, E], q_next_sel [B, M] -> (y [B], per-sample loss [B], d mean(loss) / d q [B, E])"""
    B, E = q.shape
    y = rewards + gamma * (1 - terminations) * (q_next_sel.min(axis=1) - alpha * next_logp)
    d = q - y[:, None]
    return y, (d * d).mean(axis=1), 2.0 * d / (B * E)


def policy_seed(qa):
    """redq.py:195-198: qa [B, E] -> (min_q [B], d mean(-min_q) / d qa [B, E]: jnp.min's gradient, split evenly among exact ties)"""
    B = qa.shape[0]
    mn = qa.min(axis=1)
    hit = qa == mn[:, None]
    return mn, (-hit.astype(qa.dtype) / (B * hit.sum(axis=1, keepdims=True))).astype(qa.dtype)


def critic_step(ps, qs, pp, qp, qtp, log_alpha, batch, eps1, subset, h, cs=None, cs2=None):
    """critic_loss_fn meaned (redq.py:148-176, :217-222) -> (q_loss, gcritic [E n], y [B]); batch = (s, s', a, r, term) of ONE step"""
    s, s2, a, r, term = batch
    cs = s if cs is None else cs
    cs2 = s2 if cs2 is None else cs2
    dt = qp.dtype
    E, n = int(h["ensemble_size"]), qs.n_params
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    nm, nls, _, _ = sac.policy_forward(ps, pp, s2, lo, hi)
    na, nlogp = sac.tanh_gaussian(nm, nls, eps1)
    x2 = np.concatenate([cs2, na], axis=1)
    qn = np.concatenate([nets.forward(qs, qtp[m * n:(m + 1) * n], x2)[0] for m in subset], axis=1)
    q, caches = tt.critic_forward(qs, qp, E, cs, a)
    y, loss, dq = critic_loss(q, qn, r, term, alpha, nlogp, dt.type(h["gamma"]))
    g = np.concatenate([nets.backward(qs, qp[e * n:(e + 1) * n], caches[e], dq[:, e:e + 1].astype(dt)) for e in range(E)])
    return loss.mean(), g, y


def policy_step(ps, qs, pp, qp, log_alpha, s, eps2, h, cs=None):
    """policy_entropy_loss_fn meaned (redq.py:179-215) -> (metrics, gpolicy, g_log_alpha)"""
    cs = s if cs is None else cs
    dt = pp.dtype
    B = s.shape[0]
    E, n = int(h["ensemble_size"]), qs.n_params
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    cm, cls, cls_raw, pc = sac.policy_forward(ps, pp, s, lo, hi)
    std = np.exp(cls)
    ca, clogp = sac.tanh_gaussian(cm, cls, eps2)
    entropy = -clogp
    qa, caches = tt.critic_forward(qs, qp, E, cs, ca)
    min_q, seed = policy_seed(qa)
    Oc = cs.shape[1]
    dq_da = np.zeros_like(ca)
    for e in range(E):
        _, dx = nets.backward(qs, qp[e * n:(e + 1) * n], caches[e], seed[:, e:e + 1].astype(dt), need_dx=True)
        dq_da += dx[:, Oc:]
    one_m = 1.0 - ca ** 2
    d_u = (alpha / B * 2.0 * ca / (one_m + 1e-6) + dq_da) * one_m     # alpha logp through a = tanh(u), as oracle/sac.py
    inside = (cls_raw > lo) & (cls_raw < hi)
    d_ls = np.where(inside, d_u * std * eps2 - alpha / B, 0.0)
    gpolicy = nets.backward(ps, pp, pc, np.concatenate([d_u, d_ls], axis=1).astype(dt))
    ga = alpha * (entropy - h["target_entropy"]).mean()
    metrics = {"loss/policy_loss": (alpha * clogp - min_q).mean(), "loss/entropy_loss": (alpha * (entropy - h["target_entropy"])).mean(),
               "entropy/entropy": entropy.mean(), "entropy/alpha": alpha, "q_value/q_value": min_q.mean()}
    return metrics, gpolicy, dt.type(ga)


def run_update(critic_step_i, policy_step_0, st, batch, eps1, eps2, h, lr_policy, lr_critic, lr_critic_delta, lr_alpha, tau,
               critic_states=None, critic_next_states=None):
    """The G-step driver of the REDQ, AQE and DroQ twins (redq.py:228-253), from the state st (STATE_KEYS, q_count, pi_count).
    batch: (s [G, B, O], s', a [G, B, A], r [G, B], term); eps1 [G, B, A], eps2 [B, A].  Critic step i is
    critic_step_i(i, P, Q, QT, log_alpha, batch i, eps1[i], cs[i], cs2[i]) -> (q_loss, gcritic, y), followed by Adam at lr_critic + i
    lr_critic_delta and Polyak; then policy_step_0(P, Q, log_alpha, s[0], eps2, cs[0]) -> (metrics, gpolicy, g_log_alpha).
    -> (new state, metrics, {"gq": [G] critic gradients, "gp", "ga"}, y [G, B])"""
    dt = st["P"].dtype
    c = lambda x: None if x is None else np.asarray(x, dt)
    s, s2, a, r, term = (c(x) for x in batch)
    cs, cs2 = c(critic_states), c(critic_next_states)
    eps1, eps2 = c(eps1), c(eps2)
    G = int(h["q_update_steps"])
    Q, qm, qv, QT = st["Q"], st["qm"], st["qv"], st["QT"]
    losses, norms, gqs, ys = [], [], [], []
    for i in range(G):
        loss, g, y = critic_step_i(i, st["P"], Q, QT, st["la"][0], (s[i], s2[i], a[i], r[i], term[i]), eps1[i],
                                   None if cs is None else cs[i], None if cs2 is None else cs2[i])
        Q, qm, qv = oppo.adam_step(Q, g, qm, qv, st["q_count"] + i, dt.type(np.float32(lr_critic) + np.float32(i) * np.float32(lr_critic_delta)))
        QT = sac.polyak(Q, QT, dt.type(tau))
        losses.append(loss)
        norms.append(np.linalg.norm(g))
        gqs.append(g)
        ys.append(y)
    met, gp, ga = policy_step_0(st["P"], Q, st["la"][0], s[0], eps2, None if cs is None else cs[0])
    new = {"Q": Q, "qm": qm, "qv": qv, "QT": QT, "q_count": st["q_count"] + G, "pi_count": st["pi_count"] + 1}
    new["P"], new["pm"], new["pv"] = oppo.adam_step(st["P"], gp, st["pm"], st["pv"], st["pi_count"], lr_policy)
    new["la"], new["am"], new["av"] = oppo.adam_step(st["la"], np.array([ga], dt), st["am"], st["av"], st["pi_count"], lr_alpha)
    met = dict(met)
    met.update({"loss/q_loss": np.mean(losses), "gradients/policy_grad_norm": np.linalg.norm(gp),
                "gradients/critic_grad_norm": np.mean(norms), "gradients/entropy_grad_norm": abs(float(ga))})
    return new, met, {"gq": gqs, "gp": gp, "ga": ga}, np.stack(ys)


def update(ps, qs, st, batch, eps1, eps2, subsets, h, *rates_and_critic_states):
    """`update` (redq.py:144-261): run_update's arguments with the target subsets [G, M] as one more input"""
    return run_update(lambda i, P, Q, QT, la, b, e1, cs, cs2: critic_step(ps, qs, P, Q, QT, la, b, e1, list(subsets[i]), h, cs, cs2),
                      lambda P, Q, la, s, e2, cs: policy_step(ps, qs, P, Q, la, s, e2, h, cs),
                      st, batch, eps1, eps2, h, *rates_and_critic_states)


def losses_torch(ps, pp, qs, qp, qtp, log_alpha, batch, eps1, eps2, subset, h, critic_states=None, critic_next_states=None):
    """ONE critic step's loss and the policy / entropy loss on the same parameters, restated with torch ops (float64) and
    differentiated by torch.autograd: torch.min over the stacked critics splits its gradient evenly among ties, as jnp.min does.
    -> (q_loss, gQ, policy_loss + entropy_loss, gP, gLA)"""
    import torch
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    P, Q, LA = t(pp).requires_grad_(True), t(qp).requires_grad_(True), t(log_alpha).requires_grad_(True)
    QT = t(qtp)
    A = ps.out_dim // 2
    E, n = int(h["ensemble_size"]), qs.n_params
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    s, s2, a, r, term = (t(x) for x in batch)
    cs = s if critic_states is None else t(critic_states)
    cs2 = s2 if critic_next_states is None else t(critic_next_states)

    def pol(params, x):
        out = nets.torch_forward(ps, params, x)
        return out[:, :A], torch.clamp(out[:, A:], lo, hi)

    def qvals(params, which, obs, act):
        x = torch.cat([obs, act], dim=1)
        return torch.cat([nets.torch_forward(qs, params[e * n:(e + 1) * n], x) for e in which], dim=1)

    def tg(mean, ls, eps):
        u = mean + torch.exp(ls) * eps
        act = torch.tanh(u)
        return act, (-0.5 * ((u - mean) / torch.exp(ls)) ** 2 - 0.5 * tt.LOG_2PI - ls - torch.log(1.0 - act ** 2 + 1e-6)).sum(1)

    alpha_g = torch.exp(LA)
    alpha = alpha_g.detach()
    na, nlp = tg(*pol(P.detach(), s2), t(eps1))
    y = r + h["gamma"] * (1 - term) * (qvals(QT, list(subset), cs2, na).min(dim=1).values - alpha * nlp)
    q_loss = ((qvals(Q, range(E), cs, a) - y[:, None]) ** 2).mean()
    gQ, = torch.autograd.grad(q_loss, Q)
    ca, clp = tg(*pol(P, s), t(eps2))
    entropy = (-clp).detach()
    min_q = qvals(Q.detach(), range(E), cs, ca).min(dim=1).values
    pe_loss = (alpha * clp - min_q + alpha_g * (entropy - h["target_entropy"])).mean()
    gP, gLA = torch.autograd.grad(pe_loss, (P, LA))
    return q_loss.item(), gQ.numpy(), pe_loss.item(), gP.numpy(), gLA.item()
