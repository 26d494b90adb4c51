"""Float64 numpy twin of rl-x_amd/csrc/espo.hip (ESPO, rl_x/algorithms/espo/pytorch), written from the library's flat parameter
layout (include/rlx_hip.h, rlx_mlp_desc arch A: W0[in, H], b0, W1[H, H], b1, head W[H, out], b, then the policy's logstd[out]): the
two tanh networks with hand-written backward passes, Policy.get_logprob_entropy / get_deterministic_action, GAE, one policy step
and one critic step (clip_grad_norm_ + torch.optim.Adam), and the epoch loop with its early stop.  Nothing here touches the GPU or
the library."""
import numpy as np

METRICS = ("loss/policy_gradient_loss", "loss/critic_loss", "loss/entropy_loss", "policy_ratio/ratio_delta", "policy_ratio/approx_kl",
           "gradients/policy_grad_norm", "gradients/critic_grad_norm")      # espo.py:266-274, the order of rlx_espo_update_f32's rows
HP = dict(max_ratio_delta=0.25, delta_calc_operator="mean", entropy_coef=0.0, critic_coef=0.5, max_grad_norm=0.5, learning_rate=3e-4,
          gamma=0.99, gae_lambda=0.95, adam_b1=0.9, adam_b2=0.999, adam_eps=1e-8)      # espo/pytorch/default_config.py
LOG_SQRT_2PI = float(np.log(np.sqrt(2.0 * np.pi)))


def layout(in_dim, H, out, logstd):
    L, off = {"in": in_dim, "H": H, "out": out}, 0
    for name, n in (("W0", in_dim * H), ("b0", H), ("W1", H * H), ("b1", H), ("Wh", H * out), ("bh", out)) + ((("logstd", out),) if logstd else ()):
        L[name] = (off, n)
        off += n
    L["n"] = off
    return L


def _get(p, L, name, shape):
    o, n = L[name]
    return p[o:o + n].reshape(shape)


def make_params(seed, Op, Oc, A, H, std_dev=1.0, head_std=0.3):
    """(policy flat, critic flat) of a seeded numpy generator, float32-representable: N(0, 1 / fan_in) hidden weights, small biases,
    heads N(0, head_std^2 / fan_in), logstd = log(std_dev) + 0.1 N"""
    rng = np.random.default_rng(seed)

    def net(L):
        p = np.zeros(L["n"])
        for k, fan in (("W0", L["in"]), ("W1", L["H"])):
            o, n = L[k]
            p[o:o + n] = rng.standard_normal(n) / np.sqrt(fan)
        for k in ("b0", "b1", "bh"):
            o, n = L[k]
            p[o:o + n] = 0.05 * rng.standard_normal(n)
        o, n = L["Wh"]
        p[o:o + n] = rng.standard_normal(n) * head_std / np.sqrt(L["H"])
        if "logstd" in L:
            o, n = L["logstd"]
            p[o:o + n] = np.log(std_dev) + 0.1 * rng.standard_normal(n)
        return p.astype(np.float32).astype(np.float64)
    return net(layout(Op, H, A, True)), net(layout(Oc, H, 1, False))


def forward(p, L, x):
    h0 = np.tanh(x @ _get(p, L, "W0", (L["in"], L["H"])) + _get(p, L, "b0", (L["H"],)))
    h1 = np.tanh(h0 @ _get(p, L, "W1", (L["H"], L["H"])) + _get(p, L, "b1", (L["H"],)))
    out = h1 @ _get(p, L, "Wh", (L["H"], L["out"])) + _get(p, L, "bh", (L["out"],))
    return h0, h1, out


def backward(p, L, x, h0, h1, dout):
    """flat gradient of the chain's parameters (logstd left at zero) from d out"""
    g = np.zeros(L["n"])
    H = L["H"]

    def put(name, val):
        o, n = L[name]
        g[o:o + n] = val.reshape(-1)
    put("Wh", h1.T @ dout)
    put("bh", dout.sum(0))
    dz1 = (dout @ _get(p, L, "Wh", (H, L["out"])).T) * (1.0 - h1 * h1)
    put("W1", h0.T @ dz1)
    put("b1", dz1.sum(0))
    dz0 = (dz1 @ _get(p, L, "W1", (H, H)).T) * (1.0 - h0 * h0)
    put("W0", x.T @ dz0)
    put("b0", dz0.sum(0))
    return g


def logprob_entropy(p, L, x, actions):
    """Policy.get_logprob_entropy (policy.py:57-63) -> (log_prob [n], entropy [n], mean [n, A])"""
    mean = forward(p, L, x)[2]
    logstd = _get(p, L, "logstd", (L["out"],))
    std = np.exp(logstd)
    lp = (-((actions - mean) ** 2) / (2.0 * std * std) - np.log(std) - LOG_SQRT_2PI).sum(1)
    ent = np.full(x.shape[0], (0.5 + 0.5 * np.log(2.0 * np.pi) + np.log(std)).sum())
    return lp, ent, mean


def deterministic_action(p, L, x, low, high):
    """Policy.get_deterministic_action with action_clipping_and_rescaling (policy.py:66-73)"""
    mean = forward(p, L, x)[2]
    return low + 0.5 * (np.clip(mean, -1.0, 1.0) + 1.0) * (high - low)


def gae(rewards, terminations, values, next_values, gamma, lam):
    """calculate_gae_advantages_and_returns (espo.py:112-120), [T, N] arrays"""
    delta = rewards + gamma * next_values * (1.0 - terminations) - values
    adv = np.zeros_like(rewards)
    last = np.zeros_like(rewards[0])
    for t in range(values.shape[0] - 1, -1, -1):
        last = adv[t] = delta[t] + gamma * lam * (1.0 - terminations[t]) * last
    return adv, adv + values


def clip_adam(p, g, m, v, step, lr, hp):
    """clip_grad_norm_(max_grad_norm) then torch.optim.Adam (single-tensor form); in place.  -> the norm before clipping.  A
    non-finite norm skips the step (the library's rule)."""
    norm = float(np.sqrt((g * g).sum()))
    if not np.isfinite(norm):
        return norm
    if hp["max_grad_norm"] > 0:
        g = g * min(hp["max_grad_norm"] / (norm + 1e-6), 1.0)
    b1, b2 = hp["adam_b1"], hp["adam_b2"]
    m += (g - m) * (1.0 - b1)
    v *= b2
    v += (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p -= (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + hp["adam_eps"]))
    return norm


def lower_median(x):
    """torch.median of a vector: sorted[(n - 1) // 2]; NaN when any entry is"""
    if np.isnan(x).any():
        return float("nan")
    return float(np.sort(x)[(x.size - 1) // 2])


def policy_step(p, m, v, L, x, actions, old_lp, adv, hp, step, lr):
    """policy_loss_fn (espo.py:123-141) -> dict of its five results plus the margins the fixtures' conditions are stated on"""
    h0, h1, mean = forward(p, L, x)
    logstd = _get(p, L, "logstd", (L["out"],))
    std = np.exp(logstd)
    d = actions - mean
    lp = (-(d * d) / (2.0 * std * std) - np.log(std) - LOG_SQRT_2PI).sum(1)
    logratio = lp - old_lp
    ratio = np.exp(logratio)
    kl = float(((ratio - 1.0) - logratio).mean())
    dev = np.abs(ratio - 1.0)
    median = hp["delta_calc_operator"] == "median"
    rd = lower_median(dev) if median else float(dev.mean())
    n = x.shape[0]
    an = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    pg = float((-an * ratio).mean())
    ent = float((0.5 + 0.5 * np.log(2.0 * np.pi) + np.log(std)).sum())
    coef = -an * ratio / n                                             # d loss / d logp
    g = backward(p, L, x, h0, h1, coef[:, None] * d / (std * std))
    o, k = L["logstd"]
    g[o:o + k] = (coef[:, None] * (d * d / (std * std) - 1.0)).sum(0) - hp["entropy_coef"]
    norm = clip_adam(p, g, m, v, step, lr, hp)
    s = np.sort(dev)
    gap = abs(s[n // 2] - s[n // 2 - 1]) / max(abs(s[n // 2]), 1e-300) if (median and n % 2 == 0) else np.inf
    return dict(ratio_delta=rd, pg_loss=pg, entropy=ent, approx_kl=kl, grad_norm=norm, middle_gap=gap)


def critic_step(p, m, v, L, x, returns, hp, step, lr):
    """critic_loss_fn (espo.py:146-158) -> (v_loss, grad norm)"""
    h0, h1, out = forward(p, L, x)
    dv = out[:, 0] - returns
    loss = float(hp["critic_coef"] * (0.5 * dv * dv).mean())
    g = backward(p, L, x, h0, h1, (hp["critic_coef"] * dv / x.shape[0])[:, None])
    return loss, clip_adam(p, g, m, v, step, lr, hp)


def new_state(pparams, cparams):
    z = np.zeros_like
    return dict(p=pparams.copy(), pm=z(pparams), pv=z(pparams), c=cparams.copy(), cm=z(cparams), cv=z(cparams), count=0)


def update(st, Lp, Lc, states, actions, log_probs, advantages, returns, idx, hp, lr=None, pidx=None, cidx=None):
    """The epoch loop (espo.py:236-278) on the rows idx[e] of the flat rollout, in place on `st` (new_state).
    -> (metrics [epochs_run, 7], epochs_run, info: per-epoch relative distance of ratio_delta from the threshold, middle gaps)"""
    lr = hp["learning_rate"] if lr is None else lr
    xp_all = states if pidx is None else states[:, pidx]
    xc_all = states if cidx is None else states[:, cidx]
    rows, margin, gaps = [], [], []
    for e in range(idx.shape[0]):
        mbi = idx[e]
        step = st["count"] + e + 1
        r = policy_step(st["p"], st["pm"], st["pv"], Lp, xp_all[mbi], actions[mbi], log_probs[mbi], advantages[mbi], hp, step, lr)
        cl, cn = critic_step(st["c"], st["cm"], st["cv"], Lc, xc_all[mbi], returns[mbi], hp, step, lr)
        rows.append([r["pg_loss"], cl, r["entropy"], r["ratio_delta"], r["approx_kl"], r["grad_norm"], cn])
        thr = hp["max_ratio_delta"]
        margin.append(abs(r["ratio_delta"] - thr) / abs(thr) if np.isfinite(thr) else np.inf)
        gaps.append(r["middle_gap"])
        if r["ratio_delta"] > thr:
            break
    st["count"] += len(rows)
    return np.array(rows), len(rows), dict(margin=np.array(margin), middle_gap=np.array(gaps))


def draw_indices(rng, B, mb, max_epochs):
    """the reference's draws (espo.py:241), all max_epochs of them: int32 [max_epochs, mb]"""
    return np.stack([rng.choice(B, size=mb, replace=False) for _ in range(max_epochs)]).astype(np.int32)
