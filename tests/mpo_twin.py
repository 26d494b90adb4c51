"""Float64 CPU twin of rl-x_amd/csrc/mpo.hip (MPO, rl_x/algorithms/mpo/pytorch), written from the library's flat parameter layouts
(include/rlx_hip.h, rlx_mpo_desc): the LayerNorm-tanh-ELU networks, Policy.sample_action / get_deterministic_action, and one whole
`update` (critic step, actor step, dual step with clip_grad_norm_ + Adam and the clamps).  Gradients come from torch autograd in
float64 on the CPU; nothing here touches the GPU or the library."""
import numpy as np
import torch
import torch.nn.functional as F

D = torch.float64
SOFTPLUS0 = float(np.float32(np.log(2.0)))        # float(F.softplus(torch.zeros(1))) of the float32 module (policy.py:51)
# mpo.py:114-115 compute log(S) and log(2 pi) as float32 tensors.  The twin rounds numpy's float64 log to float32 instead of
# calling torch's float32 log, which is one ulp off for some arguments on some CPU builds (log 7 on one of ours).
LOG_2PI = float(np.float32(np.log(2.0 * np.pi)))


def log_f32(x):
    return float(np.float32(np.log(float(x))))
METRICS = ("loss/critic_loss", "loss/actor_loss", "loss/dual_loss", "loss/loss_eta", "loss/loss_alpha", "q/current_q_mean", "dual/eta",
           "dual/penalty_temperature", "dual/alpha_mean", "dual/alpha_std", "kl/mean_kl_mean", "kl/mean_kl_std",
           "gradients/actor_grad_norm", "gradients/critic_grad_norm", "gradients/dual_grad_norm", "policy/std_min_mean",
           "policy/std_max_mean")      # mpo.py:389-407, the order of rlx_mpo_update_f32's metrics
HP = dict(gamma=0.99, v_min=-1600.0, v_max=1600.0, max_grad_norm=40.0, epsilon_non_parametric=0.1, epsilon_parametric_mu=0.01,
          epsilon_parametric_sigma=1e-6, epsilon_penalty=0.001, policy_init_scale=0.5, policy_min_scale=1e-6, float_epsilon=1e-8,
          min_log_temperature=-18.0, min_log_alpha=-18.0, action_sampling_number=20, action_clipping=True, action_rescaling=True,
          agent_learning_rate=3e-4, dual_learning_rate=1e-2, init_log_eta=10.0, init_log_alpha_mean=10.0, init_log_alpha_stddev=1000.0,
          init_log_penalty_temperature=10.0)     # mpo/pytorch/default_config.py


def layout(in_dim, H, out):
    L, off = {"in": in_dim, "H": H, "out": out}, 0
    for name, n in (("W0", in_dim * H), ("b0", H), ("g0", H), ("be0", H), ("W1", H * H), ("b1", H), ("W2", H * H), ("b2", H),
                    ("Wh", H * out), ("bh", out)):
        L[name] = (off, n)
        off += n
    L["n"] = off
    return L


def policy_layout(Op, A, H):
    return layout(Op, H, 2 * A)


def critic_layout(Oc, A, H, NA):
    return layout(Oc + A, H, NA)


def _get(p, L, name, shape):
    o, n = L[name]
    return p[o:o + n].reshape(shape)


def make_params(seed, Op, Oc, A, H, NA, head_std=0.3):
    """(policy flat, critic flat) of a seeded numpy generator, float32-representable: uniform +-sqrt(3 / fan_in) / 3 hidden weights
    (policy.py:54-58), LayerNorm scale 1 + 0.1 N, small biases, heads N(0, head_std^2 / fan_in)"""
    rng = np.random.default_rng(seed)

    def net(L):
        p = np.zeros(L["n"])
        for k in ("W0", "W1", "W2"):
            o, n = L[k]
            fan = L["in"] if k == "W0" else L["H"]
            p[o:o + n] = rng.uniform(-1.0, 1.0, n) * np.sqrt(3.0 / fan) * 0.333
        for k in ("b0", "b1", "b2", "be0", "bh"):
            o, n = L[k]
            p[o:o + n] = 0.05 * rng.standard_normal(n)
        o, n = L["g0"]
        p[o:o + n] = 1.0 + 0.1 * rng.standard_normal(n)
        o, n = L["Wh"]
        p[o:o + n] = rng.standard_normal(n) * head_std / np.sqrt(L["H"])
        return p.astype(np.float32).astype(np.float64)
    return net(policy_layout(Op, A, H)), net(critic_layout(Oc, A, H, NA))


def init_duals(A, hp):
    return np.array([hp["init_log_eta"]] + [hp["init_log_alpha_mean"]] * A + [hp["init_log_alpha_stddev"]] * A +
                    [hp["init_log_penalty_temperature"]], np.float32).astype(np.float64)


def net_fwd(p, L, x):
    """trunk + head: Linear -> LayerNorm(1e-5) -> tanh -> Linear -> ELU -> Linear -> ELU -> head"""
    H, i, o = L["H"], L["in"], L["out"]
    z = x @ _get(p, L, "W0", (i, H)) + _get(p, L, "b0", (H,))
    h = torch.tanh(F.layer_norm(z, (H,), _get(p, L, "g0", (H,)), _get(p, L, "be0", (H,)), eps=1e-5))
    h = F.elu(h @ _get(p, L, "W1", (H, H)) + _get(p, L, "b1", (H,)))
    h = F.elu(h @ _get(p, L, "W2", (H, H)) + _get(p, L, "b2", (H,)))
    return h @ _get(p, L, "Wh", (H, o)) + _get(p, L, "bh", (o,))


def policy_get_action(p, L, x, hp):
    """Policy.get_action (policy.py:71-77) -> (mean, std)"""
    out = net_fwd(p, L, x)
    A = L["out"] // 2
    return out[:, :A], hp["policy_min_scale"] + (F.softplus(out[:, A:]) * hp["policy_init_scale"] / SOFTPLUS0)


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64), dtype=D)


def act(p, L, obs, eps, hp, low, high, deterministic=False):
    """Policy.sample_action / get_deterministic_action (policy.py:80-97) -> (action, processed action)"""
    with torch.no_grad():
        mean, std = policy_get_action(_t(p), L, _t(obs), hp)
        a = mean if deterministic else mean + std * _t(eps)
        pa = torch.clamp(a, -1.0, 1.0) if hp["action_clipping"] else a
        if hp["action_rescaling"]:
            pa = _t(low) + (0.5 * (pa + 1.0) * (_t(high) - _t(low)))
    return a.numpy(), pa.numpy()


def clip_adam(p, g, m, v, step, lr, max_norm, mask=None, b1=0.9, b2=0.999, eps=1e-8):
    """clip_grad_norm_ (over the entries that have a gradient) + torch.optim.Adam (single-tensor form) -> (p, m, v, norm)"""
    mask = np.ones(p.size, bool) if mask is None else mask
    norm = float(np.sqrt(np.sum(g[mask] ** 2)))
    if max_norm > 0:
        g = g * min(max_norm / (norm + 1e-6), 1.0)
    m2, v2 = m * b1 + (1 - b1) * g, v * b2 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p2 = p - (lr / bc1) * m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps)
    return np.where(mask, p2, p), np.where(mask, m2, m), np.where(mask, v2, v), norm


def _critic(q, LQ, x, a, clip):
    if clip:
        a = torch.clamp(a, -1.0, 1.0)
    return net_fwd(q, LQ, torch.cat([x, a], dim=1))


def update(st, LP, LQ, batch, eps_c, eps_a, hp, step, pidx=None, cidx=None):
    """One `update` (mpo.py:124-267).  st: dict of float64 numpy vectors p, pm, pv, tp, q, qm, qv, tq, d, dm, dv (targets read only);
    batch = (states, next_states, actions, rewards, dones, truncations, effective_n_steps); eps_c [S, B, A], eps_a [S, 2B, A].
    Returns (new state dict, metrics[17], extras)."""
    s, s2, a, r, dn, tr, ns = (_t(x) for x in batch)
    sp = (lambda x: x[:, pidx]) if pidx is not None else (lambda x: x)
    sc = (lambda x: x[:, cidx]) if cidx is not None else (lambda x: x)
    S, B, A, NA = hp["action_sampling_number"], s.shape[0], LP["out"] // 2, LQ["out"]
    clip, feps = bool(hp["action_clipping"]), hp["float_epsilon"]
    z = torch.linspace(hp["v_min"], hp["v_max"], NA, dtype=D)
    log_s = log_f32(S)
    tp, tq = _t(st["tp"]), _t(st["tq"])
    # ---- critic step (mpo.py:125-156)
    with torch.no_grad():
        mt, sdt = policy_get_action(tp, LP, sp(s2), hp)
        sa = mt[None] + sdt[None] * _t(eps_c)
        lg = _critic(tq, LQ, sc(s2).repeat(S, 1), sa.reshape(-1, A), clip).view(S, B, NA)
        pmf = F.softmax(lg, dim=-1)
        disc = (hp["gamma"] ** ns) * (1.0 - dn * (1.0 - tr))
        tz = torch.clamp(r[:, None] + disc[:, None] * z[None], hp["v_min"], hp["v_max"])
        proj = torch.clamp(1.0 - (tz[:, None, :] - z[None, :, None]).abs() / (z[1] - z[0]), 0.0, 1.0)   # [B, i, j]
        tpmf = torch.einsum("bij,sbj->bi", proj, pmf) / S           # = mean_s sum_j proj pmf_s (mpo.py:145-147)
    q = _t(st["q"]).requires_grad_(True)
    cl = _critic(q, LQ, sc(s), a, clip)
    cq = (F.softmax(cl, dim=-1) * z).sum(-1)
    q_loss = -torch.sum(tpmf * F.log_softmax(cl, dim=1), dim=1).mean()
    gq = torch.autograd.grad(q_loss, q)[0].numpy()
    q_new, qm, qv, cnorm = clip_adam(st["q"], gq, st["qm"], st["qv"], step, hp["agent_learning_rate"], hp["max_grad_norm"])
    # ---- actor step (mpo.py:158-236)
    ss = torch.cat([s, s2], dim=0)
    R = 2 * B
    with torch.no_grad():
        mt, sdt = policy_get_action(tp, LP, sp(ss), hp)
        sa = mt[None] + sdt[None] * _t(eps_a)
        Q = (F.softmax(_critic(tq, LQ, sc(ss).repeat(S, 1), sa.reshape(-1, A), clip).view(S, R, NA), dim=-1) * z).sum(-1)
    d = _t(st["d"]).requires_grad_(True)
    log_eta, la_std, lpt = d[0], d[1 + A:1 + 2 * A], d[1 + 2 * A]
    eta = F.softplus(log_eta) + feps
    w = F.softmax(Q / eta.detach(), dim=0)
    loss_eta = eta * (hp["epsilon_non_parametric"] + torch.logsumexp(Q / eta, dim=0).mean() - log_s)
    w_q = w
    if clip:
        pt = F.softplus(lpt) + feps
        cost = -torch.linalg.norm(sa - torch.clamp(sa, -1.0, 1.0), dim=-1)
        w = w + F.softmax(cost / pt.detach(), dim=0)
        loss_eta = loss_eta + pt * (hp["epsilon_penalty"] + torch.logsumexp(cost / pt, dim=0).mean() - log_s)
        ptd = float(pt.detach())
    else:
        ptd = 0.0
    p = _t(st["p"]).requires_grad_(True)
    mo, so = policy_get_action(p, LP, sp(ss), hp)
    alpha = torch.logaddexp(la_std, torch.zeros_like(la_std)) + feps     # mpo.py:202-203: both from log_alpha_stddev
    lpm = torch.sum(-0.5 * ((((sa - mo) / sdt) ** 2) + LOG_2PI) - torch.log(sdt), dim=-1)
    loss_pg_mean = -(lpm * w).sum(dim=0).mean()
    s0 = torch.clamp(sdt, min=feps)
    kl_mean = torch.log(s0 / s0) + (s0 ** 2 + (mt - mo) ** 2) / (2.0 * s0 ** 2) - 0.5
    mkm = kl_mean.mean(dim=0)
    loss_kl_mean = torch.sum(alpha.detach() * mkm)
    loss_alpha_mean = torch.sum(alpha * (hp["epsilon_parametric_mu"] - mkm.detach()))
    lps = torch.sum(-0.5 * ((((sa - mt) / so) ** 2) + LOG_2PI) - torch.log(so), dim=-1)
    loss_pg_std = -(lps * w).sum(dim=0).mean()
    s1 = torch.clamp(so, min=feps)
    kl_std = torch.log(s1 / s0) + (s0 ** 2 + (mt - mt) ** 2) / (2.0 * s1 ** 2) - 0.5
    mks = kl_std.mean(dim=0)
    loss_kl_std = torch.sum(alpha.detach() * mks)
    loss_alpha_std = torch.sum(alpha * (hp["epsilon_parametric_sigma"] - mks.detach()))
    actor_loss = loss_pg_mean + loss_pg_std + loss_kl_mean + loss_kl_std
    gp = torch.autograd.grad(actor_loss, p)[0].numpy()
    p_new, pm, pv, anorm = clip_adam(st["p"], gp, st["pm"], st["pv"], step, hp["agent_learning_rate"], hp["max_grad_norm"])
    # ---- dual step (mpo.py:238-247): log_alpha_mean has no gradient; log_penalty_temperature only with action_clipping
    dual_loss = loss_alpha_mean + loss_alpha_std + loss_eta
    gd = torch.autograd.grad(dual_loss, d)[0].numpy()
    mask = np.ones(2 * A + 2, bool)
    mask[1:1 + A] = False
    mask[1 + 2 * A] = clip
    d_new, dm, dv, dnorm = clip_adam(st["d"], gd, st["dm"], st["dv"], step, hp["dual_learning_rate"], hp["max_grad_norm"], mask)
    d_new = d_new.copy()
    d_new[0] = max(d_new[0], hp["min_log_temperature"])
    d_new[1:1 + 2 * A] = np.maximum(d_new[1:1 + 2 * A], hp["min_log_alpha"])
    det = lambda x: float(x.detach())
    metrics = np.array([det(q_loss), det(actor_loss), det(dual_loss), det(loss_eta), det(loss_alpha_mean) + det(loss_alpha_std),
                        det(cq.mean()), det(eta), ptd, det(alpha.mean()), det(alpha.mean()), det(mkm.mean()), det(mks.mean()), anorm,
                        cnorm, dnorm, det(so.min(dim=1).values.mean()), det(so.max(dim=1).values.mean())])
    new = dict(st, p=p_new, pm=pm, pv=pv, q=q_new, qm=qm, qv=qv, d=d_new, dm=dm, dv=dv)
    extras = {"weights": w.detach().numpy(), "weights_q": w_q.detach().numpy(), "gp": gp, "gq": gq, "gd": gd,
              "target_pmf": tpmf.numpy(), "q": Q.numpy()}
    return new, metrics, extras
