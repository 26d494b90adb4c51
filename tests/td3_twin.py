"""CPU twin (test infrastructure) of td3.hip: the reference's TD3 and DDPG updates restated in numpy, written from
rl_x/algorithms/td3/flax/td3.py:106-205 (policy.py:22-44, critic.py:17-53) and rl_x/algorithms/ddpg/flax/ddpg.py:104-166.

  acting        td3.py:107-112   a = clip(tanh(pi(s)) + epsilon n, -1, 1); processed = low + 0.5 (clip(a) + 1)(high - low)
  critic step   td3.py:116-160   a' = clip(tanh(pi_target(s')) + clip(smoothing_epsilon n, +-smoothing_clip_value), -1, 1);
                                 y = r + gamma (1 - term) min_e Q_target,e(s', a'); loss = mean over batch AND critics of (q_e - y)^2;
                                 plain Adam of the critics; the targets stay
  policy step   td3.py:164-199   loss = mean(-min_e Q_e(s, pi(s))) on the critics as they are NOW (after the critic step); jnp.min's
                                 gradient, split evenly among exact ties; plain Adam of the policy; Polyak of the critics AND the policy
  ddpg step     ddpg.py:114-166  one critic, no noise; q_loss + policy_loss differentiated at the SAME (pre-step) parameters, the
                                 policy's gradient through stop_gradient(critic_params); both Adam steps, both Polyak steps

The noise is an INPUT: the key chain (split(key, B + 1), row i <-> keys[1 + i]) is checked separately against oracle/prng.py.
Built on oracle/nets.py (networks, the hand-written reverse pass) and oracle/sac.py (lecun init, Polyak), oracle/ppo.py (optax.adam).
The reference's TD3 and DDPG exist in JAX only and JAX is not installed: PARITY UNPINNED by the reference; tests/test_td3_twin.py
pins the twin with hand-computed answers and float64 torch.autograd.

Q matrices here are [B, E] (column e = critic e); the library's are [E, B].  The dtype of the state is the dtype of the whole
evaluation: float64 for the reference values, float32 to measure what float32 arithmetic itself costs (tests/test_gpu_td3.py).
"""
import numpy as np

from oracle import nets, ppo as oppo, sac

STATE_KEYS = ("P", "pm", "pv", "PT", "Q", "qm", "qv", "QT")
METRICS = ("loss/q_loss", "gradients/critic_grad_norm", "loss/policy_loss", "q_value/q_value", "gradients/policy_grad_norm")


def make_specs(policy_obs_dim, critic_obs_dim, act_dim, policy_hidden, critic_hidden):
    """policy.py:22-44 (the tanh is applied by the callers), critic.py:17-30"""
    ps = nets.MLPSpec(policy_obs_dim, policy_hidden, act_dim, nets.ACT_RELU, False, False)
    qs = nets.MLPSpec(critic_obs_dim + act_dim, critic_hidden, 1, nets.ACT_RELU, False, False)
    return ps, qs


def zero_state(pp, ptp, qp, qtp, dtype=np.float64):
    f = lambda x: np.asarray(x, np.float32).astype(dtype)
    z = np.zeros_like
    return {"P": f(pp), "pm": z(f(pp)), "pv": z(f(pp)), "PT": f(ptp), "Q": f(qp), "qm": z(f(qp)), "qv": z(f(qp)), "QT": f(qtp),
            "q_count": 0, "pi_count": 0}


def cast_state(st, dtype):
    """the float32 VALUES of st in `dtype`"""
    return {k: (np.asarray(v, np.float32).astype(dtype) if k in STATE_KEYS else v) for k, v in st.items()}


def problem(seed, O, A, B, ph, qh, E=2, Oc=None, head_scale=1.0):
    """tests/redq_twin.py's input recipe (float32 values: lecun init + 0.02 noise, targets = online + 0.01 noise) with a policy target
    -> dict(ps, qs, state (float64), batch, cbatch or None, h)"""
    rng = np.random.default_rng(seed)
    ps, qs = make_specs(O, O if Oc is None else Oc, A, ph, qh)
    pp = (sac.lecun_normal_init(ps, rng) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    pp[ps.head["W"]:ps.head["W"] + ps.head["in"] * ps.head["out"]] *= head_scale
    ptp = (pp + 0.01 * rng.standard_normal(pp.shape)).astype(np.float32)
    qp = (np.concatenate([sac.lecun_normal_init(qs, rng) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params)).astype(np.float32)
    qtp = (qp + 0.01 * rng.standard_normal(qp.shape)).astype(np.float32)
    f = lambda x: x.astype(np.float32)
    batch = (f(rng.standard_normal((B, O))), f(rng.standard_normal((B, O))), f(np.tanh(rng.standard_normal((B, A)))),
             f(rng.standard_normal(B)), f(rng.random(B) < 0.2))
    cbatch = None if Oc is None else (f(rng.standard_normal((B, Oc))), f(rng.standard_normal((B, Oc))))
    h = dict(gamma=0.99, smoothing_epsilon=0.2, smoothing_clip_value=0.5, nr_critics=E)
    return dict(ps=ps, qs=qs, state=zero_state(pp, ptp, qp, qtp), batch=batch, cbatch=cbatch, h=h)


def critic_forward(qs, qp, E, obs, act):
    """-> q [B, E], the E caches"""
    n = qs.n_params
    x = np.concatenate([obs, act], axis=1)
    outs, caches = zip(*(nets.forward(qs, qp[e * n:(e + 1) * n], x) for e in range(E)))
    return np.concatenate(outs, axis=1), caches


def act(ps, pp, obs, noise, epsilon, low, high):
    """get_action (td3.py:107-112) and get_processed_action (policy.py:39-44) -> (action, processed action); epsilon 0: deterministic"""
    dt = pp.dtype
    a = np.tanh(nets.forward(ps, pp, np.asarray(obs, dt))[0])
    if epsilon != 0:
        a = np.clip(a + dt.type(epsilon) * np.asarray(noise, dt), -1.0, 1.0)
    low, high = np.asarray(low, dt), np.asarray(high, dt)
    return a, low + 0.5 * (np.clip(a, -1.0, 1.0) + 1.0) * (high - low)


def target_action(ps, ptp, s2, noise, h, inner_clip=True):
    """td3.py:125-128; noise None: DDPG's (ddpg.py:122).  inner_clip False: a FAULT for tests/test_td3_cases.py (the noise unclipped)"""
    dt = ptp.dtype
    a = np.tanh(nets.forward(ps, ptp, s2)[0])
    if noise is None:
        return a
    nz = np.asarray(noise, dt) * dt.type(h["smoothing_epsilon"])
    if inner_clip:
        nz = np.clip(nz, -dt.type(h["smoothing_clip_value"]), dt.type(h["smoothing_clip_value"]))
    return np.clip(a + nz, -1.0, 1.0)


def critic_loss(q, q_next, rewards, terminations, gamma):
    """td3.py:130-134 for a batch: q, q_next [B, E] -> (y [B], per-sample loss [B], d mean(loss) / d q [B, E])"""
    B, E = q.shape
    y = rewards + gamma * (1 - terminations) * q_next.min(axis=1)
    d = q - y[:, None]
    return y, (d * d).mean(axis=1), 2.0 * d / (B * E)


def policy_seed(qa, use_min=True):
    """td3.py:170-172: qa [B, E] -> (min_q [B], d mean(-min_q) / d qa [B, E]: jnp.min's gradient, split evenly among exact ties).
    use_min False: a FAULT for tests/test_td3_cases.py (critic 0 in place of the min)"""
    B = qa.shape[0]
    if not use_min:
        seed = np.zeros_like(qa)
        seed[:, 0] = -1.0 / B
        return qa[:, 0], seed
    mn = qa.min(axis=1)
    hit = qa == mn[:, None]
    return mn, (-hit.astype(qa.dtype) / (B * hit.sum(axis=1, keepdims=True))).astype(qa.dtype)


def critic_grads(ps, qs, PT, Q, QT, batch, noise, h, cs=None, cs2=None, inner_clip=True):
    """the critic loss meaned (td3.py:120-154) at the given parameters -> (q_loss, gcritic [E n], aux: y, q, q_next, next_action, dq)"""
    s, s2, a, r, term = batch
    cs = s if cs is None else cs
    cs2 = s2 if cs2 is None else cs2
    dt = Q.dtype
    E, n = int(h["nr_critics"]), qs.n_params
    na = target_action(ps, PT, s2, noise, h, inner_clip)
    qn, _ = critic_forward(qs, QT, E, cs2, na)
    q, caches = critic_forward(qs, Q, E, cs, a)
    y, loss, dq = critic_loss(q, qn, r, term, dt.type(h["gamma"]))
    g = np.concatenate([nets.backward(qs, Q[e * n:(e + 1) * n], caches[e], dq[:, e:e + 1].astype(dt)) for e in range(E)])
    return loss.mean(), g, dict(y=y, q=q, q_next=qn, next_action=na, dq=dq)


def policy_grads(ps, qs, P, Q, s, h, cs=None, use_min=True):
    """the policy loss meaned (td3.py:167-188) at the given parameters -> (metrics, gpolicy, aux: qa, seed, action)"""
    cs = s if cs is None else cs
    dt = P.dtype
    E, n = int(h["nr_critics"]), qs.n_params
    head, pc = nets.forward(ps, P, s)
    ca = np.tanh(head)
    qa, caches = critic_forward(qs, Q, E, cs, ca)
    min_q, seed = policy_seed(qa, use_min)
    Oc = cs.shape[1]
    dq_da = np.zeros_like(ca)
    for e in range(E):
        _, dx = nets.backward(qs, Q[e * n:(e + 1) * n], caches[e], seed[:, e:e + 1].astype(dt), need_dx=True)
        dq_da += dx[:, Oc:]
    gp = nets.backward(ps, P, pc, (dq_da * (1.0 - ca ** 2)).astype(dt))
    return {"loss/policy_loss": (-min_q).mean(), "q_value/q_value": min_q.mean()}, gp, dict(qa=qa, seed=seed, action=ca)


def _batch(st, batch, cs, cs2):
    dt = st["P"].dtype
    c = lambda x: None if x is None else np.asarray(x, dt)
    return tuple(c(x) for x in batch), c(cs), c(cs2)


def critic_step(ps, qs, st, batch, noise, h, lr_critic, critic_states=None, critic_next_states=None, inner_clip=True):
    """update_critic (td3.py:116-160) from the state st -> (new state, metrics, aux incl. gq and y).  The targets do not move."""
    b, cs, cs2 = _batch(st, batch, critic_states, critic_next_states)
    loss, g, aux = critic_grads(ps, qs, st["PT"], st["Q"], st["QT"], b, None if noise is None else np.asarray(noise, st["P"].dtype), h, cs, cs2,
                                inner_clip)
    new = dict(st)
    new["Q"], new["qm"], new["qv"] = oppo.adam_step(st["Q"], g, st["qm"], st["qv"], st["q_count"], lr_critic)
    new["q_count"] = st["q_count"] + 1
    return new, {"loss/q_loss": loss, "gradients/critic_grad_norm": np.linalg.norm(g)}, dict(aux, gq=g)


def policy_step(ps, qs, st, states, h, lr_policy, tau, critic_states=None, use_min=True):
    """update_policy_and_targets (td3.py:164-199) from the state st (whose critics the critic step has already moved)
    -> (new state, metrics, aux incl. gp)"""
    dt = st["P"].dtype
    s = np.asarray(states, dt)
    cs = None if critic_states is None else np.asarray(critic_states, dt)
    met, gp, aux = policy_grads(ps, qs, st["P"], st["Q"], s, h, cs, use_min)
    new = dict(st)
    new["P"], new["pm"], new["pv"] = oppo.adam_step(st["P"], gp, st["pm"], st["pv"], st["pi_count"], lr_policy)
    new["QT"] = sac.polyak(st["Q"], st["QT"], dt.type(tau))
    new["PT"] = sac.polyak(new["P"], st["PT"], dt.type(tau))
    new["pi_count"] = st["pi_count"] + 1
    return new, dict(met, **{"gradients/policy_grad_norm": np.linalg.norm(gp)}), dict(aux, gp=gp)


def update(ps, qs, st, batch, noise, h, lr_policy, lr_critic, tau, do_policy_step=True, critic_states=None, critic_next_states=None,
           inner_clip=True, use_min=True, move_targets_always=False):
    """one vector step's optimisation (td3.py:278-290): the critic step, then -- when the delay allows -- the policy step and the
    targets.  move_targets_always: a FAULT for tests/test_td3_cases.py (Polyak on a critic-only step)
    -> (new state, metrics, aux of both steps)"""
    new, met, aux = critic_step(ps, qs, st, batch, noise, h, lr_critic, critic_states, critic_next_states, inner_clip)
    if do_policy_step:
        new, pmet, paux = policy_step(ps, qs, new, batch[0], h, lr_policy, tau, critic_states, use_min)
        met, aux = dict(met, **pmet), dict(aux, **paux)
    elif move_targets_always:
        dt = st["P"].dtype
        new["QT"], new["PT"] = sac.polyak(new["Q"], new["QT"], dt.type(tau)), sac.polyak(new["P"], new["PT"], dt.type(tau))
    return new, met, aux


def ddpg_step(ps, qs, st, batch, h, lr_policy, lr_critic, tau, critic_states=None, critic_next_states=None):
    """DDPG's `update` (ddpg.py:114-166): both gradients at the parameters of st, then both Adam steps, then both Polyak steps
    -> (new state, metrics, aux)"""
    assert int(h["nr_critics"]) == 1
    dt = st["P"].dtype
    b, cs, cs2 = _batch(st, batch, critic_states, critic_next_states)
    loss, gq, aux = critic_grads(ps, qs, st["PT"], st["Q"], st["QT"], b, None, h, cs, cs2)
    pmet, gp, paux = policy_grads(ps, qs, st["P"], st["Q"], b[0], h, cs)
    new = dict(st)
    new["P"], new["pm"], new["pv"] = oppo.adam_step(st["P"], gp, st["pm"], st["pv"], st["pi_count"], lr_policy)
    new["Q"], new["qm"], new["qv"] = oppo.adam_step(st["Q"], gq, st["qm"], st["qv"], st["q_count"], lr_critic)
    new["QT"] = sac.polyak(new["Q"], st["QT"], dt.type(tau))
    new["PT"] = sac.polyak(new["P"], st["PT"], dt.type(tau))
    new["q_count"], new["pi_count"] = st["q_count"] + 1, st["pi_count"] + 1
    met = dict(pmet, **{"loss/q_loss": loss, "gradients/critic_grad_norm": np.linalg.norm(gq), "gradients/policy_grad_norm": np.linalg.norm(gp)})
    return new, met, dict(aux, **paux, gq=gq, gp=gp)


def losses_torch(ps, qs, P, PT, Q, QT, batch, noise, h, critic_states=None, critic_next_states=None, joint=False):
    """the critic loss and the policy loss restated with torch ops (float64) and differentiated by torch.autograd: torch.min over
    the stacked critics splits its gradient evenly among ties, as jnp.min does.  joint: DDPG's one loss (ddpg.py:134), differentiated
    once with respect to both parameter vectors.  -> (q_loss, gQ, policy_loss, gP)"""
    import torch
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    Pt, Qt = t(P).requires_grad_(True), t(Q).requires_grad_(True)
    E, n = int(h["nr_critics"]), qs.n_params
    s, s2, a, r, term = (t(x) for x in batch)
    cs = s if critic_states is None else t(critic_states)
    cs2 = s2 if critic_next_states is None else t(critic_next_states)

    def qvals(params, obs, act):
        x = torch.cat([obs, act], dim=1)
        return torch.cat([nets.torch_forward(qs, params[e * n:(e + 1) * n], x) for e in range(E)], dim=1)

    na = torch.tanh(nets.torch_forward(ps, t(PT), s2))
    if noise is not None:
        nz = torch.clamp(t(noise) * h["smoothing_epsilon"], -h["smoothing_clip_value"], h["smoothing_clip_value"])
        na = torch.clamp(na + nz, -1.0, 1.0)
    y = r + h["gamma"] * (1 - term) * qvals(t(QT), cs2, na).min(dim=1).values
    q_loss = ((qvals(Qt, cs, a) - y[:, None]) ** 2).mean()
    policy_loss = (-qvals(Qt.detach(), cs, torch.tanh(nets.torch_forward(ps, Pt, s))).min(dim=1).values).mean()
    if joint:
        gP, gQ = torch.autograd.grad(q_loss + policy_loss, (Pt, Qt))
    else:
        gQ, = torch.autograd.grad(q_loss, Qt)
        gP, = torch.autograd.grad(policy_loss, Pt)
    return q_loss.item(), gQ.numpy(), policy_loss.item(), gP.numpy()


def smoothing_noise(key, B, A, partitionable=True):
    """the update's key chain (td3.py:149-150, :126): keys = split(key, B + 1); -> (keys[0], noise [B, A] with row i = normal(keys[1 + i], (A,)))"""
    from oracle import prng
    ks = prng.split(np.asarray(key, np.uint32), B + 1, partitionable)
    return ks[0], np.stack([prng.normal(k, (A,), partitionable) for k in ks[1:]])


def acting_noise(key, N, A, partitionable=True):
    """get_action's (td3.py:108-110): key, sub = split(key); -> (key, normal(sub, (N, A))): ONE shape-wide draw"""
    from oracle import prng
    ks = prng.split(np.asarray(key, np.uint32), 2, partitionable)
    return ks[0], prng.normal(ks[1], (N, A), partitionable)
