"""CPU restatement of FastSAC's networks and update steps -- TEST INFRASTRUCTURE ONLY (oracle/__init__.py).

Follows rl_x/algorithms/fastsac/pytorch:
    policy.py:46-57     torso Linear(O,512)-LayerNorm-SiLU, Linear(512,256)-LayerNorm-SiLU, Linear(256,128)-LayerNorm-SiLU
                        (torch.nn.LayerNorm: population variance, eps 1e-5), heads mean / log_std Linear(128, A)
    policy.py:66-72     log_std = min + 0.5 (max - min) (tanh(raw) + 1)
    policy.py:75-90     a = tanh(mean + std eps) * action_scale;  log_prob = sum_j Normal(mean, std).log_prob(raw)
                        - log(1 - tanh^2 + 1e-6) - log(action_scale + 1e-6)
    policy.py:36-43     action_scale = max(|low - center|, |high - center|) / scale
    q_network.py:27-43  critic Linear(Oc + A,768)-LN-SiLU, Linear(768,384)-LN-SiLU, Linear(384,192)-LN-SiLU, Linear(192, nr_atoms)
    fastsac.py:144-241  critic_and_entropy_loss_fn: next action / log-prob from the policy (no gradient), categorical projection
                        of the entropy-adjusted n-step target (oracle/c51.py restates it), q_loss = q1_loss + q2_loss,
                        AdamW step of both critics; entropy_loss = mean(exp(log_alpha) (entropy - target_entropy)) with
                        entropy = -next_log_probs, AdamW step of log_alpha
    fastsac.py:323-327  Polyak: target = (1 - tau) target + tau param, every parameter of both critics
    fastsac.py:106-141  policy_loss_fn: loss = mean(alpha log_prob - q) with q = (q1 + q2) / 2 (or min) of the EXPECTED values
                        sum_j softmax(logits)_j z_j; AdamW step of the policy
    fastsac.py:88-91    torch.optim.AdamW(lr, weight_decay, betas): p *= 1 - lr wd; m, v moments; p -= lr / (1 - b1^t) * m /
                        (sqrt(v) / sqrt(1 - b2^t) + 1e-8)

Parameters live in the library's flat layout (include/rlx_hip.h, rlx_lnmlp_desc): per hidden layer W[in, out] row-major, b,
LayerNorm scale, LayerNorm bias; then the head W[in, out], b.  The policy's head is [mean | log_std], 2A wide.

The widths above are the defaults (POLICY_HIDDEN / CRITIC_HIDDEN); make_params, policy_forward, critic_logits, critic_step and
policy_step take other ones (policy_hidden= / critic_hidden=) and the critics' own observation columns (critic_batch= /
critic_states=) for the shape tests; critic_update / policy_update add clip_grad_norm_, AdamW, Polyak and the log_alpha step.

Pinned by tests/golden/reference_fastsac.npz: outputs of the reference's own modules and closures executed in float64
(tests/golden/make_reference_golden.py: make_fastsac), checked in tests/test_oracle_fastsac.py."""
import math

import numpy as np
import torch

from oracle import c51

POLICY_HIDDEN = (512, 256, 128)
CRITIC_HIDDEN = (768, 384, 192)
LN_EPS = 1e-5


def param_count(in_dim, hidden, out_dim):
    n, d = 0, in_dim
    for h in hidden:
        n += d * h + 3 * h
        d = h
    return n + d * out_dim + out_dim


def blocks(in_dim, hidden, out_dim):
    """[(name, offset, size)] of the flat layout."""
    out, off, d = [], 0, in_dim
    for li, h in enumerate(hidden):
        for name, n in (("W%d" % li, d * h), ("b%d" % li, h), ("g%d" % li, h), ("be%d" % li, h)):
            out.append((name, off, n))
            off += n
        d = h
    out += [("Wh", off, d * out_dim), ("bh", off + d * out_dim, out_dim)]
    return out


def make_params(seed, obs_dim, act_dim, nr_atoms, critic_obs_dim=None, policy_hidden=POLICY_HIDDEN, critic_hidden=CRITIC_HIDDEN):
    """Deterministic test parameters in the flat layout: (policy, [q1, q2, q1_target, q2_target]) float32 arrays drawn from
    numpy's PCG64 -- the fixture generator loads exactly these into the reference's modules, a test rebuilds them from the seed.
    policy_hidden / critic_hidden: other hidden widths than the reference's (the shape tests)."""
    rng = np.random.default_rng(seed)
    oc = obs_dim if critic_obs_dim is None else critic_obs_dim

    def net(in_dim, hidden, out_dim, head_scale):
        parts, d = [], in_dim
        for h in hidden:
            parts += [rng.standard_normal((d, h)) / np.sqrt(d), 0.1 * rng.standard_normal(h), 1.0 + 0.1 * rng.standard_normal(h),
                      0.1 * rng.standard_normal(h)]
            d = h
        parts += [head_scale * rng.standard_normal((d, out_dim)) / np.sqrt(d), 0.1 * rng.standard_normal(out_dim)]
        return np.concatenate([x.reshape(-1) for x in parts]).astype(np.float32)
    policy = net(obs_dim, policy_hidden, 2 * act_dim, 0.5)
    critics = [net(oc + act_dim, critic_hidden, nr_atoms, 1.0) for _ in range(4)]
    return policy, critics


def forward(flat, in_dim, hidden, out_dim, x, keep=None):
    """flat, x: torch tensors (any float dtype).  -> head output [M, out_dim].  keep (a list) receives (z_l, h_l) per layer; a
    z_l that takes part in a backward keeps its gradient (z_l.grad after it)."""
    off, d, h = 0, in_dim, x
    for width in hidden:
        W = flat[off:off + d * width].reshape(d, width); off += d * width
        b = flat[off:off + width]; off += width
        g = flat[off:off + width]; off += width
        be = flat[off:off + width]; off += width
        z = h @ W + b
        mean = z.mean(dim=1, keepdim=True)
        var = ((z - mean) ** 2).mean(dim=1, keepdim=True)
        y = (z - mean) / torch.sqrt(var + LN_EPS) * g + be
        h = y * torch.sigmoid(y)
        if keep is not None:
            if z.requires_grad:
                z.retain_grad()
            keep.append((z, h))
        d = width
    W = flat[off:off + d * out_dim].reshape(d, out_dim); off += d * out_dim
    b = flat[off:off + out_dim]
    return h @ W + b


def policy_forward(pflat, obs_dim, act_dim, obs, log_std_min, log_std_max, policy_hidden=POLICY_HIDDEN, keep=None):
    head = forward(pflat, obs_dim, policy_hidden, 2 * act_dim, obs, keep)
    mean, raw = head[:, :act_dim], head[:, act_dim:]
    log_std = log_std_min + 0.5 * (log_std_max - log_std_min) * (torch.tanh(raw) + 1.0)
    return mean, log_std


def sample(mean, log_std, eps, action_scale):
    """-> (scaled action, log-prob) as policy.get_action_and_log_prob computes them for the noise eps."""
    std = torch.exp(log_std)
    raw = mean + std * eps
    t = torch.tanh(raw)
    logp = -((raw - mean) ** 2) / (2.0 * std * std) - log_std - math.log(math.sqrt(2.0 * math.pi))
    # (policy.py:36-43 builds action_scale from float32 tensors and it is no module buffer: it STAYS float32 whatever the module's
    #  dtype, so this one term is float32 arithmetic in the reference).  The float32 log is taken as the correctly rounded one:
    #  torch's own float32 log comes from a vector-math library whose last bit depends on the CPU it runs on, and one ulp
    #  here moves a Q value by ~5e-9 (tests/test_oracle_fastsac.py asserts 1e-10 relative)
    x32 = action_scale.to(torch.float32) + 1e-6
    log_scale = torch.log(x32.to(torch.float64)).to(torch.float32).to(mean.dtype)
    logp = logp - torch.log((1.0 - t * t) + 1e-6) - log_scale
    return t * action_scale, logp.sum(dim=1)


def critic_logits(qflat, obs_dim, act_dim, nr_atoms, obs, act, critic_hidden=CRITIC_HIDDEN, keep=None):
    return forward(qflat, obs_dim + act_dim, critic_hidden, nr_atoms, torch.cat([obs, act], dim=1), keep)


def adamw(p, g, m, v, step, lr, weight_decay, b1, b2, eps=1e-8):
    """One torch.optim.AdamW step (numpy arrays, `step` 1-based).  -> (p, m, v)."""
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


def clip_grad_norm(g, max_norm):
    """torch.nn.utils.clip_grad_norm_ on one flat gradient vector (fastsac.py:129-130, :218-219): g * min(1, c / (norm + 1e-6));
    returns (clipped gradient, the UN-clipped norm -- what the reference logs).  max_norm == -1: no clipping (fastsac.py:131-136)."""
    norm = float(np.linalg.norm(g))
    if max_norm == -1.0:
        return g, norm
    return g * min(1.0, max_norm / (norm + 1e-6)), norm


def polyak(target, params, tau):
    return (1.0 - tau) * target + tau * params


def critic_step(pflat, q1, q2, t1, t2, log_alpha, obs_dim, act_dim, nr_atoms, batch, noise_next, action_scale, hp, clipped,
                critic_batch=None, policy_hidden=POLICY_HIDDEN, critic_hidden=CRITIC_HIDDEN, dtype=np.float64, trace=None):
    """batch = (states, next_states, actions, rewards, dones, truncations, n_steps), numpy float64, with the POLICY's observation
    columns; critic_batch = (critic states, critic next states) or None (the same columns).  obs_dim: the critic's observation
    width (the policy's is the batch's).  dtype: the precision the whole step is evaluated in (np.float32: what float32 alone
    costs).  trace (a list): receives [input rows, (z_l, h_l) per hidden layer] of every network forward, in call order.
    -> dict(q_loss, q_min, q_max, entropy, entropy_loss, g_q1, g_q2, g_log_alpha, next_log_probs)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=dtype))
    def keep(x):                                  # a fresh per-forward list in `trace`, or None
        if trace is None:
            return None
        trace.append([x])
        return trace[-1]
    s, s2, a, rew, done, trunc, nst = (t(x) for x in batch)
    cs, cs2 = (s, s2) if critic_batch is None else (t(critic_batch[0]), t(critic_batch[1]))
    scale = t(action_scale)
    with torch.no_grad():
        mean, ls = policy_forward(t(pflat), s2.shape[1], act_dim, s2, hp["log_std_min"], hp["log_std_max"], policy_hidden, keep(s2))
        a2, lp2 = sample(mean, ls, t(noise_next), scale)
        x2 = torch.cat([cs2, a2], dim=1)
        nl1 = critic_logits(t(t1), obs_dim, act_dim, nr_atoms, cs2, a2, critic_hidden, keep(x2)).numpy()
        nl2 = critic_logits(t(t2), obs_dim, act_dim, nr_atoms, cs2, a2, critic_hidden, keep(x2)).numpy()
    alpha = math.exp(log_alpha)
    args = (rew.numpy(), done.numpy(), trunc.numpy(), nst.numpy(), lp2.numpy(), alpha, hp["gamma"], hp["v_min"], hp["v_max"])
    p1, v1 = c51.project(nl1, *args)
    p2, v2 = c51.project(nl2, *args)
    if clipped:
        sel = np.where((v1 < v2)[:, None], p1, p2)
        tgt1 = tgt2 = sel
    else:
        tgt1, tgt2 = p1, p2
    Q1, Q2 = t(q1).requires_grad_(True), t(q2).requires_grad_(True)
    x1 = torch.cat([cs, a], dim=1)
    l1 = critic_logits(Q1, obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, keep(x1))
    l2 = critic_logits(Q2, obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, keep(x1))
    loss = -(t(tgt1) * torch.log_softmax(l1, dim=1)).sum(dim=1).mean() - (t(tgt2) * torch.log_softmax(l2, dim=1)).sum(dim=1).mean()
    loss.backward()
    entropy = -lp2.numpy()
    return dict(q_loss=float(loss.detach()), q_min=float(v1.min()), q_max=float(v1.max()), entropy=float(entropy.mean()),
                entropy_loss=float((alpha * (entropy - hp["target_entropy"])).mean()), g_q1=Q1.grad.numpy(), g_q2=Q2.grad.numpy(),
                g_log_alpha=float(alpha * (entropy - hp["target_entropy"]).mean()), next_log_probs=lp2.numpy(),
                q1_logits=l1.detach().numpy(), q2_logits=l2.detach().numpy())


def policy_step(pflat, q1, q2, log_alpha, obs_dim, act_dim, nr_atoms, states, noise_cur, action_scale, hp, clipped, critic_states=None,
                policy_hidden=POLICY_HIDDEN, critic_hidden=CRITIC_HIDDEN, trace=None):
    """states: the POLICY's observation columns; critic_states: the critics' (None: the same); obs_dim: the critic's width.
    trace: as in critic_step.  -> dict(policy_loss, g_policy, log_probs, q_value)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    def keep(x):
        if trace is None:
            return None
        trace.append([x])
        return trace[-1]
    s, scale = t(states), t(action_scale)
    cs = s if critic_states is None else t(critic_states)
    P = t(pflat).requires_grad_(True)
    mean, ls = policy_forward(P, s.shape[1], act_dim, s, hp["log_std_min"], hp["log_std_max"], policy_hidden, keep(s))
    a, lp = sample(mean, ls, t(noise_cur), scale)
    z = torch.linspace(hp["v_min"], hp["v_max"], nr_atoms, dtype=torch.float64)
    xa = torch.cat([cs, a], dim=1)
    v1 = (torch.softmax(critic_logits(t(q1), obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, keep(xa)), dim=1) * z).sum(dim=1)
    v2 = (torch.softmax(critic_logits(t(q2), obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, keep(xa)), dim=1) * z).sum(dim=1)
    q = torch.minimum(v1, v2) if clipped else (v1 + v2) / 2.0
    loss = (math.exp(log_alpha) * lp - q).mean()
    loss.backward()
    return dict(policy_loss=float(loss.detach()), g_policy=P.grad.numpy(), log_probs=lp.detach().numpy(), q_value=q.detach().numpy(),
                actions=a.detach().numpy())


def critic_update(pflat, qparams, qm, qv, qtarget, log_alpha, am, av, step, obs_dim, act_dim, nr_atoms, batch, noise_next, action_scale,
                  hp, clipped, critic_batch=None, **kw):
    """critic_step + clip_grad_norm_ + AdamW over both critics (flat [q1 | q2]) + Polyak + the AdamW step of log_alpha (the
    critic step used alpha BEFORE it).  step: 1-based optimizer step; hp["max_grad_norm"] (default -1: no clipping).
    -> (qparams, qm, qv, qtarget, log_alpha, am, av, metrics [q_loss, entropy_loss, q_min, q_max, entropy, critic_grad_norm,
    entropy_grad_norm ** 2 (what the reference logs), alpha before the step], critic_step dict)"""
    nq = qparams.size // 2
    r = critic_step(pflat, qparams[:nq], qparams[nq:], qtarget[:nq], qtarget[nq:], log_alpha, obs_dim, act_dim, nr_atoms, batch, noise_next,
                    action_scale, hp, clipped, critic_batch, **kw)
    b1, b2, lr, wd = hp["adam_beta1"], hp["adam_beta2"], hp["learning_rate"], hp["weight_decay"]
    g, norm = clip_grad_norm(np.concatenate([r["g_q1"], r["g_q2"]]), hp.get("max_grad_norm", -1.0))
    qp, qm, qv = adamw(np.asarray(qparams, np.float64), g, qm, qv, step, lr, wd, b1, b2)
    qt = polyak(np.asarray(qtarget, np.float64), qp, hp["tau"])
    la, am, av = adamw(np.float64(log_alpha), r["g_log_alpha"], np.float64(am), np.float64(av), step, lr, wd, b1, b2)
    met = np.array([r["q_loss"], r["entropy_loss"], r["q_min"], r["q_max"], r["entropy"], norm, r["g_log_alpha"] ** 2, math.exp(log_alpha)])
    return qp, qm, qv, qt, float(la), float(am), float(av), met, r


def policy_update(pflat, pm, pv, step, qparams, log_alpha, obs_dim, act_dim, nr_atoms, states, noise_cur, action_scale, hp, clipped,
                  critic_states=None, **kw):
    """policy_step + clip_grad_norm_ + AdamW.  -> (pparams, pm, pv, metrics [policy_loss, alpha, policy_grad_norm], policy_step dict)"""
    nq = qparams.size // 2
    r = policy_step(pflat, qparams[:nq], qparams[nq:], log_alpha, obs_dim, act_dim, nr_atoms, states, noise_cur, action_scale, hp, clipped,
                    critic_states, **kw)
    g, norm = clip_grad_norm(r["g_policy"], hp.get("max_grad_norm", -1.0))
    pp, pm, pv = adamw(np.asarray(pflat, np.float64), g, pm, pv, step, hp["learning_rate"], hp["weight_decay"], hp["adam_beta1"],
                       hp["adam_beta2"])
    return pp, pm, pv, np.array([r["policy_loss"], math.exp(log_alpha), norm]), r


def nstep_sample(ring, pos, size, capacity, n_steps, gamma, idx_t, idx_e):
    """ReplayBuffer.sample (replay_buffer.py:34-96) for GIVEN start rows idx_t and env columns idx_e (the reference draws them with
    torch.randint).  ring = dict(states, next_states, actions, rewards, dones, truncations) of [capacity, nr_envs, ...] numpy arrays.
    -> (states, next_states, actions, rewards, dones, truncations, effective_n_steps)."""
    B = idx_t.shape[0]
    if n_steps == 1:
        g = lambda k: ring[k][idx_t, idx_e]
        return g("states"), g("next_states"), g("actions"), g("rewards"), g("dones"), g("truncations"), np.ones(B, ring["dones"].dtype)
    trunc = ring["truncations"]
    if size >= capacity:
        trunc = trunc.copy()
        last = (pos - 1) % capacity
        trunc[last] = np.where(ring["dones"][last] > 0.0, trunc[last], 1.0)
    all_t = (idx_t[:, None] + np.arange(n_steps)[None, :]) % capacity
    env = np.broadcast_to(idx_e[:, None], all_t.shape)
    rew, dn, tr = ring["rewards"][all_t, env], ring["dones"][all_t, env], trunc[all_t, env]
    shifted = np.concatenate([np.zeros((B, 1), dn.dtype), dn[:, :-1]], axis=1)
    masks = np.cumprod(1.0 - shifted, axis=1)
    eff = masks.sum(axis=1)
    disc = (np.asarray(gamma, dtype=np.float32) ** np.arange(n_steps, dtype=np.float32)).astype(rew.dtype)
    rewards = (rew * masks * disc[None, :]).sum(axis=1)
    first = lambda x: np.where((x > 0.0).sum(axis=1) == 0, n_steps - 1, np.argmax(x > 0.0, axis=1))
    final = np.minimum(first(dn), first(tr))
    ft = all_t[np.arange(B), final]
    return (ring["states"][idx_t, idx_e], ring["next_states"][ft, idx_e], ring["actions"][idx_t, idx_e], rewards, ring["dones"][ft, idx_e],
            trunc[ft, idx_e], eff)
