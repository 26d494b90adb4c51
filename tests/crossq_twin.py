"""CPU twin (test infrastructure) of brn.hip: the reference's batch renormalisation layer restated in numpy with a hand-written
backward, written from rl_x/algorithms/crossq/flax/batch_renorm.py:77-130.  It is the column-statistics layer CrossQ's networks are
made of (crossq/flax/critic.py:25-60, policy.py:34-72); below it the two networks, the critic update (crossq.py:147-206), the policy
and entropy update (:210-274), acting (:135-143), optax-style Adam and the key chain from oracle/prng.py.  The noise is an INPUT of
the updates.

  eval   :87-93    y = (x - ra_mean) rsqrt(ra_var + eps) g + b
  train  :95-128   mu, v = max(0, mean x^2 - mu^2) (flax's fast variance); r, d clipped and under stop_gradient; w = 1 once the
                   layer's `steps` has reached warm_up_steps; cm = mu - w d sqrt(v) / r (no eps under this sqrt); cv = v s with
                   s = w / r^2 + 1 - w; y = (x - cm) rsqrt(cv + eps) g + b; then the running statistics advance

The backward of a training pass (derived by hand; tests/test_crossq_twin.py holds it against float64 torch.autograd with both clips
active and inactive): S1 = sum dY g, S2 = sum dY g (x - cm), dcm = -rho S1, dcv = -rho^3 S2 / 2, dv = dcv s - w dcm d / (2 sqrt(v) r),
dX = dY g rho + dcm / M + dv 2 (x - mu) / M, dg = sum dY (x - cm) rho, db = sum dY.

ZERO BATCH VARIANCE: the reference's sqrt(v) has an infinite derivative at v = 0 (its autodiff gives 0 inf = NaN there); the library
and this twin take that term's gradient as 0 where w = 0 or v = 0.

The reference's CrossQ exists in JAX only and JAX is not installed: PARITY UNPINNED by the reference.  The dtype of x is the dtype of
the whole evaluation; the constants are taken through float32, as the library receives them.

FLOAT32 MODES.  A float32 evaluation is what separates float32 rounding from a wrong kernel (tests/test_gpu_crossq.py F32_GAP).  Plain
float32 (dsum=False) takes the column sums and the one-pass variance in float32 too, which brn.hip does not: k_brn_colsum and
k_brn_finish_* accumulate and do the per-column arithmetic in double because float loses it (at 4096 rows the plain mode is 2e-4 off
in the critics' first moments).  dsum=True is float32 AS THE KERNELS ACCUMULATE: mu, v, the clips, cm, s, rho, t, sdy, sdyx, dg, db
and the statistics update in float64, cast to float32 where the kernels store float32 (rho, s, t, the coefficients of the element-wise
passes, dg, db, the statistics; mu and cm stay float pairs, i.e. double); the element-wise passes and the GEMMs in float32.  On float64
inputs dsum changes nothing that is computed."""
import numpy as np

EPS, R_MAX, D_MAX, MOMENTUM = 1e-3, 3.0, 5.0, 0.99


class BrnCfg:
    def __init__(self, momentum=MOMENTUM, eps=EPS, r_max=R_MAX, d_max=D_MAX):
        self.momentum, self.eps, self.r_max, self.d_max = (float(np.float32(v)) for v in (momentum, eps, r_max, d_max))


def brn_eval(x, g, b, ra_mean, ra_var, cfg, dsum=False):
    """-> (y, cache): the running statistics as they are; nothing advances.  (dsum: an eval pass has no column sums; the flag only
    reaches the backward's dg and db)"""
    dt = x.dtype
    rho = (1.0 / np.sqrt(ra_var + dt.type(cfg.eps))).astype(dt)
    y = ((x - ra_mean) * rho * g + b).astype(dt)
    return y, {"train": False, "dsum": dsum, "x": x, "g": g, "cm": ra_mean.astype(dt), "rho": rho}


def brn_batch_stats(x):
    """-> (mu, v) [D] over the rows of x, flax's fast variance"""
    mu = x.mean(axis=0)
    return mu, np.maximum(0, (x * x).mean(axis=0) - mu * mu)


def brn_clips(mu, v, ra_mean, ra_var, cfg):
    """-> (r_raw, d_raw, r, d): the correction factors before and after their clips"""
    dt = mu.dtype
    sig = np.sqrt(ra_var + dt.type(cfg.eps))
    r_raw = np.sqrt(v + dt.type(cfg.eps)) / sig
    d_raw = (mu - ra_mean) / sig
    return r_raw, d_raw, np.clip(r_raw, dt.type(1.0 / cfg.r_max), dt.type(cfg.r_max)), np.clip(d_raw, dt.type(-cfg.d_max), dt.type(cfg.d_max))


def _pair(v, dt):
    """a float64 vector as brn.hip's float pair -> (hi, lo) in dt"""
    hi = v.astype(dt)
    return hi, (v - hi.astype(np.float64)).astype(dt)


def brn_train_dsum(x, g, b, ra_mean, ra_var, cfg, warmed):
    """brn_train as k_brn_colsum / k_brn_finish_fwd / k_brn_apply_fwd compute it on x of a narrower type: the column sums and the
    per-column arithmetic in float64, the element-wise pass in x's type"""
    dt, f8 = x.dtype, np.float64
    x8 = x.astype(f8)
    mu, v = brn_batch_stats(x8)
    ram, rav = ra_mean.astype(f8), ra_var.astype(f8)
    r_raw, d_raw, r, d = brn_clips(mu, v, ram, rav, cfg)
    w = 1.0 if warmed else 0.0
    sq = np.sqrt(v)
    cm = mu - w * d * sq / r
    s = w / (r * r) + (1 - w)
    rho = 1.0 / np.sqrt(v * s + cfg.eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where((w > 0) & (v > 0), (d / r) / (2 * sq), 0)
    cm_hi, cm_lo = _pair(cm, dt)
    y = (((x - cm_hi) - cm_lo) * (rho * g.astype(f8)).astype(dt) + b).astype(dt)
    m = cfg.momentum
    cache = {"train": True, "dsum": True, "x": x, "g": g, "mu": mu, "v": v, "r": r, "d": d, "cm": cm_hi.astype(f8) + cm_lo.astype(f8),
             "s": s.astype(dt), "rho": rho.astype(dt), "t": t.astype(dt), "r_raw": r_raw, "d_raw": d_raw}
    return y, cache, (m * ram + (1 - m) * mu).astype(dt), (m * rav + (1 - m) * v).astype(dt)


def brn_backward_dsum(dY, cache, relu_mask=False):
    """brn_backward as k_brn_colsum<BWD> / k_brn_finish_bwd / k_brn_apply_bwd compute it"""
    x, g = cache["x"], cache["g"]
    dt, f8 = x.dtype, np.float64
    M = x.shape[0]
    x8, dY8, g8 = x.astype(f8), dY.astype(f8), g.astype(f8)
    sdy, sdyx = dY8.sum(axis=0), (dY8 * x8).sum(axis=0)
    cm, rho = cache["cm"].astype(f8), cache["rho"].astype(f8)
    dX = dY * (g8 * rho).astype(dt)
    if cache["train"]:
        S1, S2 = g8 * sdy, g8 * (sdyx - cm * sdy)
        dcm, dcv = -rho * S1, -0.5 * rho ** 3 * S2
        dv = dcv * cache["s"].astype(f8) - dcm * cache["t"].astype(f8)
        mu_hi, mu_lo = _pair(cache["mu"], dt)
        dX = dX + ((2 * dv / M).astype(dt) * ((x - mu_hi) - mu_lo) + (dcm / M).astype(dt))
    if relu_mask:
        dX = dX * (x > 0)
    return dX.astype(dt), (rho * (sdyx - cm * sdy)).astype(dt), sdy.astype(dt)


def brn_train(x, g, b, ra_mean, ra_var, cfg, warmed, dsum=False):
    """-> (y, cache, new_ra_mean, new_ra_var).  dsum: see FLOAT32 MODES"""
    dt = x.dtype
    if dsum and dt != np.float64:
        return brn_train_dsum(x, g, b, ra_mean, ra_var, cfg, warmed)
    mu, v = brn_batch_stats(x)
    r_raw, d_raw, r, d = brn_clips(mu, v, ra_mean, ra_var, cfg)
    w = dt.type(1.0 if warmed else 0.0)
    sq = np.sqrt(v)
    cm = (mu - w * d * sq / r).astype(dt)
    s = (w / (r * r) + (1 - w)).astype(dt)
    rho = (1.0 / np.sqrt(v * s + dt.type(cfg.eps))).astype(dt)
    y = ((x - cm) * rho * g + b).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where((w > 0) & (v > 0), (d / r) / (2 * sq), 0).astype(dt)     # the zero-variance rule
    m = dt.type(cfg.momentum)
    cache = {"train": True, "x": x, "g": g, "mu": mu, "v": v, "r": r, "d": d, "cm": cm, "s": s, "rho": rho, "t": t, "r_raw": r_raw,
             "d_raw": d_raw}
    return y, cache, (m * ra_mean + (1 - m) * mu).astype(dt), (m * ra_var + (1 - m) * v).astype(dt)


def brn_backward(dY, cache, relu_mask=False, keep_sqrt_term=True):
    """-> (dX, dg, db).  relu_mask: x is a ReLU's output and dX carries its derivative 1[x > 0].  keep_sqrt_term=False drops the
    gradient of cm's sqrt(v) term everywhere (what the zero-variance rule does on a constant column)."""
    x, g, cm, rho = cache["x"], cache["g"], cache["cm"], cache["rho"]
    dt = x.dtype
    if cache.get("dsum") and dt != np.float64:
        assert keep_sqrt_term
        return brn_backward_dsum(dY, cache, relu_mask)
    M = x.shape[0]
    xc = x - cm
    db = dY.sum(axis=0)
    dg = ((dY * xc).sum(axis=0) * rho).astype(dt)
    dX = dY * (g * rho)
    if cache["train"]:
        S1 = g * db
        S2 = g * (dY * xc).sum(axis=0)
        dcm = -rho * S1
        dcv = -0.5 * rho ** 3 * S2
        dv = dcv * cache["s"] - (dcm * cache["t"] if keep_sqrt_term else 0)
        dX = dX + dcm / M + dv * 2 * (x - cache["mu"]) / M
    if relu_mask:
        dX = dX * (x > 0)
    return dX.astype(dt), dg, db.astype(dt)


# ------------------------------------------------------------------------------------------------------------ the networks
METRICS = ("loss/q_loss", "loss/policy_loss", "loss/entropy_loss", "entropy/entropy", "entropy/alpha", "q_value/q_value",
           "gradients/policy_grad_norm", "gradients/critic_grad_norm", "gradients/entropy_grad_norm")
STATE_KEYS = ("pp", "pm", "pv", "ps", "qp", "qm", "qv", "qs", "la", "am", "av")
LOG_2PI = float(np.log(2 * np.pi))


class NetSpec:
    """offsets of one network (critic.py:25-60, policy.py:34-72): BRN l (l = 0 .. L) over D(l) columns, Dense l maps D(l) -> D(l + 1),
    Dense L is the head.  FLAT LAYOUT: bn0.scale[in], bn0.bias[in], W1[in, H1], b1, bn1.scale, bn1.bias, W2, b2, ..., W_head, b_head;
    the running statistics in a vector of their own: bn0.mean, bn0.var, bn1.mean, bn1.var, ..."""

    def __init__(self, in_dim, hidden, out_dim):
        self.in_dim, self.hidden, self.out_dim = int(in_dim), [int(h) for h in hidden], int(out_dim)
        self.L = len(self.hidden)
        self.dims = [self.in_dim] + self.hidden + [self.out_dim]
        off, so, self.bn, self.W, self.b, self.st = 0, 0, [], [], [], []
        for l in range(self.L + 1):
            D, nxt = self.dims[l], self.dims[l + 1]
            self.bn.append(off); off += 2 * D
            self.W.append(off); off += D * nxt
            self.b.append(off); off += nxt
            self.st.append(so); so += 2 * D
        self.n_params, self.n_stats = off, so

    def init(self, rng):
        """scale 1, bias 0, lecun-normal kernels, zero Dense biases -> float64 [n_params]"""
        p = np.zeros(self.n_params)
        for l in range(self.L + 1):
            D, nxt = self.dims[l], self.dims[l + 1]
            p[self.bn[l]:self.bn[l] + D] = 1.0
            p[self.W[l]:self.W[l] + D * nxt] = rng.standard_normal(D * nxt) / np.sqrt(D)
        return p

    def fresh_stats(self):
        s = np.zeros(self.n_stats)
        for l in range(self.L + 1):
            s[self.st[l] + self.dims[l]:self.st[l] + 2 * self.dims[l]] = 1.0
        return s


def net_forward(spec, p, stats, x, train, warmed, cfg, groups=None, dsum=False):
    """-> (head output [M, out], caches, new statistics).  groups: row slices normalised SEPARATELY in a training pass (None: the
    whole batch together, as the reference does; the statistics then advance from the first group)"""
    dt = x.dtype
    caches, new_stats, h = [], stats.copy(), x
    for l in range(spec.L + 1):
        D, nxt = spec.dims[l], spec.dims[l + 1]
        g, b = p[spec.bn[l]:spec.bn[l] + D], p[spec.bn[l] + D:spec.bn[l] + 2 * D]
        m0, v0 = stats[spec.st[l]:spec.st[l] + D], stats[spec.st[l] + D:spec.st[l] + 2 * D]
        if not train:
            y, bc = brn_eval(h, g, b, m0, v0, cfg, dsum)
            bcs = [(slice(None), bc)]
        else:
            y, bcs = np.empty_like(h), []
            for i, rows in enumerate(groups or [slice(None)]):
                y[rows], bc, m1, v1 = brn_train(h[rows], g, b, m0, v0, cfg, warmed, dsum)
                bcs.append((rows, bc))
                if i == 0:
                    new_stats[spec.st[l]:spec.st[l] + D], new_stats[spec.st[l] + D:spec.st[l] + 2 * D] = m1, v1
        W, bias = p[spec.W[l]:spec.W[l] + D * nxt].reshape(D, nxt), p[spec.b[l]:spec.b[l] + nxt]
        z = (y @ W + bias).astype(dt)
        caches.append({"brn": bcs, "y": y, "W": W})
        h = np.maximum(z, 0).astype(dt) if l < spec.L else z
    return h, caches, new_stats


def net_backward(spec, caches, d_out, zero_rows_below_last_brn=None):
    """-> (flat gradient, d L / d x).  zero_rows_below_last_brn: rows whose gradient is zeroed below the last BRN (what a backward
    over the first B rows alone would compute: WRONG, the batch statistics couple all rows)"""
    dt = d_out.dtype
    grads, d = np.zeros(spec.n_params, dt), d_out
    for l in range(spec.L, -1, -1):
        D, nxt, c = spec.dims[l], spec.dims[l + 1], caches[l]
        grads[spec.W[l]:spec.W[l] + D * nxt] = (c["y"].T @ d).reshape(-1)
        grads[spec.b[l]:spec.b[l] + nxt] = d.sum(axis=0)
        dY = (d @ c["W"].T).astype(dt)
        dX, dg, db = np.empty_like(dY), np.zeros(D, dt), np.zeros(D, dt)
        for rows, bc in c["brn"]:
            dX[rows], g1, b1 = brn_backward(dY[rows], bc, relu_mask=l > 0)
            dg, db = dg + g1, db + b1
        grads[spec.bn[l]:spec.bn[l] + D], grads[spec.bn[l] + D:spec.bn[l] + 2 * D] = dg, db
        if l == spec.L and zero_rows_below_last_brn is not None:
            dX[zero_rows_below_last_brn] = 0
        d = dX
    return grads, d


def train_pass_margins(caches, cfg):
    """over every layer of a training pass -> (smallest batch variance, smallest relative distance of an unclipped r or d from its
    edges): what a parity case asserts before it trusts float32 to take the same branches"""
    vmin, margin = np.inf, np.inf
    for c in caches:
        for _, bc in c["brn"]:
            vmin = min(vmin, float(bc["v"].min()))
            for raw, edges in ((bc["r_raw"], (1 / cfg.r_max, cfg.r_max)), (bc["d_raw"], (-cfg.d_max, cfg.d_max))):
                for edge in edges:
                    margin = min(margin, float(np.abs(raw - edge).min() / abs(edge)))
    return vmin, margin


# ------------------------------------------------------------------------------------------------------------ the updates
def sample(head, eps, ls_min, ls_max):
    """policy.py / crossq.py:160-166: -> (a, logp, std, inside) from the head output [B, 2 A] and the block draw eps [B, A]"""
    dt = head.dtype
    A = head.shape[1] // 2
    mean, raw = head[:, :A], head[:, A:]
    ls = np.clip(raw, dt.type(ls_min), dt.type(ls_max))
    std = np.exp(ls)
    a = np.tanh(mean + std * eps)
    logp = (-0.5 * eps * eps - dt.type(0.5 * LOG_2PI) - ls - np.log(1 - a * a + dt.type(1e-6))).sum(axis=1)
    return a.astype(dt), logp.astype(dt), std, (raw > ls_min) & (raw < ls_max)


def adam(p, g, m, v, t, lr, b1, b2, eps):
    """optax.adam, step t (from 1) -> (p, m, v)"""
    dt = p.dtype
    b1, b2, lr, eps = dt.type(np.float32(b1)), dt.type(np.float32(b2)), dt.type(np.float32(lr)), dt.type(np.float32(eps))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return (p - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)).astype(dt), m.astype(dt), v.astype(dt)


def hparams(A, E=2, warmup=100000, **kw):
    """default_config.py's values"""
    h = dict(gamma=0.99, target_entropy=-float(A), log_std_min=-20.0, log_std_max=2.0, lr_policy=1e-3, lr_critic=1e-3, lr_alpha=1e-3,
             policy_adam_b1=0.5, critic_adam_b1=0.5, alpha_adam_b1=0.9, adam_b2=0.999, adam_eps=1e-8, brn_momentum=MOMENTUM, brn_eps=EPS,
             brn_r_max=R_MAX, brn_d_max=D_MAX, brn_warmup_steps=warmup, ensemble_size=E)
    h.update(kw)
    return h


def cfg_of(h):
    return BrnCfg(h["brn_momentum"], h["brn_eps"], h["brn_r_max"], h["brn_d_max"])


def critic_update(ps, qs, st, batch, cbatch, eps, h, variant=None, dsum=False):
    """crossq.py:147-206 -> (new state, metrics, info).  batch = (s, s', a, r, term); cbatch = (cs, cs') or None; eps [B, A].
    variant: None, "zero_next_rows" (the next-state rows' gradients zeroed below the last BRN) or "separate_halves" (the two halves
    normalised separately): two wrong implementations a device result must be far from"""
    dt = st["qp"].dtype
    s, s2, a, r, term = (np.asarray(x).astype(dt) for x in batch)
    cs, cs2 = (s, s2) if cbatch is None else (np.asarray(x).astype(dt) for x in cbatch)
    B, E, cfg = s.shape[0], h["ensemble_size"], cfg_of(h)
    alpha = np.exp(st["la"][0])
    head, _, _ = net_forward(ps, st["pp"], st["ps"], s2, False, False, cfg, dsum=dsum)
    a2, logp2, _, _ = sample(head, eps.astype(dt), h["log_std_min"], h["log_std_max"])
    x = np.concatenate([np.concatenate([cs, a], axis=1), np.concatenate([cs2, a2], axis=1)], axis=0)
    warmed = st["q_count"] >= h["brn_warmup_steps"]
    groups = [slice(0, B), slice(B, 2 * B)] if variant == "separate_halves" else None
    outs, caches, new_qs = [], [], []
    for e in range(E):
        o, c, ns = net_forward(qs, st["qp"][e * qs.n_params:(e + 1) * qs.n_params], st["qs"][e * qs.n_stats:(e + 1) * qs.n_stats], x, True, warmed,
                               cfg, groups, dsum)
        outs.append(o[:, 0]); caches.append(c); new_qs.append(ns)
    q = np.stack(outs, axis=1)                                                     # [2 B, E]
    y = r + dt.type(np.float32(h["gamma"])) * (1 - term) * (q[B:].min(axis=1) - alpha * logp2)
    diff = q[:B] - y[:, None]
    q_loss = (diff * diff).mean()
    g = []
    for e in range(E):
        d = np.zeros((2 * B, 1), dt)
        d[:B, 0] = 2 * diff[:, e] / (B * E)
        g.append(net_backward(qs, caches[e], d, slice(B, 2 * B) if variant == "zero_next_rows" else None)[0])
    g = np.concatenate(g)
    new = dict(st)
    new["qp"], new["qm"], new["qv"] = adam(st["qp"], g, st["qm"], st["qv"], st["q_count"] + 1, h["lr_critic"], h["critic_adam_b1"], h["adam_b2"],
                                           h["adam_eps"])
    new["qs"] = np.concatenate(new_qs).astype(dt)
    new["q_count"] = st["q_count"] + 1
    margins = [train_pass_margins(c, cfg) for c in caches]
    info = {"grad": g, "q": q, "y": y, "a2": a2, "logp2": logp2, "vmin": min(m[0] for m in margins), "margin": min(m[1] for m in margins),
            "warmed": warmed}
    return new, {"loss/q_loss": float(q_loss), "gradients/critic_grad_norm": float(np.sqrt((g * g).sum()))}, info


def policy_update(ps, qs, st, batch, cbatch, eps, h, dsum=False):
    """crossq.py:210-274 -> (new state, metrics, info)"""
    dt = st["pp"].dtype
    s = np.asarray(batch[0]).astype(dt)
    cs = s if cbatch is None else np.asarray(cbatch[0]).astype(dt)
    B, E, cfg = s.shape[0], h["ensemble_size"], cfg_of(h)
    A = ps.out_dim // 2
    eps = eps.astype(dt)
    la = st["la"][0]
    alpha = np.exp(la)
    warmed = st["pi_count"] >= h["brn_warmup_steps"]
    head, pc, new_ps = net_forward(ps, st["pp"], st["ps"], s, True, warmed, cfg, dsum=dsum)
    a, logp, std, inside = sample(head, eps, h["log_std_min"], h["log_std_max"])
    x = np.concatenate([cs, a], axis=1)
    qa, qc = [], []
    for e in range(E):
        o, c, _ = net_forward(qs, st["qp"][e * qs.n_params:(e + 1) * qs.n_params], st["qs"][e * qs.n_stats:(e + 1) * qs.n_stats], x, False, False, cfg,
                              dsum=dsum)
        qa.append(o[:, 0]); qc.append(c)
    qa = np.stack(qa, axis=1)
    mn = qa.min(axis=1)
    ties = (qa == mn[:, None])
    seed = -(ties / ties.sum(axis=1, keepdims=True)) / B
    dqa = np.zeros((B, A), dt)
    for e in range(E):
        dqa += net_backward(qs, qc[e], seed[:, e:e + 1].astype(dt))[1][:, -A:]
    om = 1 - a * a
    du = (alpha / B * 2 * a / (om + dt.type(1e-6)) + dqa) * om
    d_head = np.concatenate([du, np.where(inside, du * std * eps - alpha / B, 0)], axis=1).astype(dt)
    g, _ = net_backward(ps, pc, d_head)
    entropy = -logp.mean()
    ga = alpha * (entropy - dt.type(np.float32(h["target_entropy"])))
    t = st["pi_count"] + 1
    new = dict(st)
    new["pp"], new["pm"], new["pv"] = adam(st["pp"], g, st["pm"], st["pv"], t, h["lr_policy"], h["policy_adam_b1"], h["adam_b2"], h["adam_eps"])
    new["la"], new["am"], new["av"] = adam(st["la"], np.array([ga], dt), st["am"], st["av"], t, h["lr_alpha"], h["alpha_adam_b1"], h["adam_b2"],
                                           h["adam_eps"])
    new["ps"] = new_ps.astype(dt)
    new["pi_count"] = t
    vmin, margin = train_pass_margins(pc, cfg)
    met = {"loss/policy_loss": float(alpha * logp.mean() - mn.mean()), "loss/entropy_loss": float(ga), "entropy/entropy": float(entropy),
           "entropy/alpha": float(alpha), "q_value/q_value": float(mn.mean()), "gradients/policy_grad_norm": float(np.sqrt((g * g).sum())),
           "gradients/entropy_grad_norm": float(abs(ga))}
    return new, met, {"grad": g, "vmin": vmin, "margin": margin, "warmed": warmed, "a": a, "logp": logp}


def act(ps, pp, pstats, obs, eps, h, deterministic=False):
    """crossq.py:135-143: the policy in eval mode -> actions [N, A]"""
    head, _, _ = net_forward(ps, pp, pstats, obs, False, False, cfg_of(h))
    return sample(head, np.zeros_like(eps) if deterministic else eps.astype(obs.dtype), h["log_std_min"], h["log_std_max"])[0]


def key_chain(key, shape, partitionable=True):
    """key, subkey = split(key); normal(subkey, shape) -> (new key, block draw): oracle/prng.py alone"""
    from oracle import prng
    ks = prng.split(key, 2, partitionable)
    return ks[0], prng.normal(ks[1], shape, partitionable=partitionable)


def problem(seed, O, A, B, ph, qh, E, Oc=None, warmup=100000, stats_away=False, dense_bias=0.0):
    """a case: float32 values -- init() + 0.02 noise on everything (so no BRN scale is exactly 1, no bias 0), policy head kernel
    scaled by 0.1, log_alpha = -0.3 -> dict(ps, qs, state (float64), batch, cbatch, h).  dense_bias is added to every hidden Dense
    bias (a case of few rows keeps its ReLU units alive with it).  stats_away: running statistics away from the batch's, so that a
    warmed case has clips that act: input column c is of kind c mod 5 -- inside both clips, r below / above its edges (running
    variance 30 / 0.02), d below / above (running mean +- 8 deviations away) -- the scales of the d-clipped columns are 0.2, and the hidden layers'
    statistics lie around what a ReLU of a unit normal plus dense_bias has, within a factor two"""
    rng = np.random.default_rng(seed)
    ps, qs = NetSpec(O, ph, 2 * A), NetSpec((O if Oc is None else Oc) + A, qh, 1)
    f = lambda v: v.astype(np.float32)
    pp = f(ps.init(rng) + 0.02 * rng.standard_normal(ps.n_params))
    pp[ps.W[ps.L]:ps.W[ps.L] + ps.dims[ps.L] * 2 * A] *= 0.1
    qp = f(np.concatenate([qs.init(rng) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params))
    for spec, v, n in ((ps, pp, 1), (qs, qp, E)):
        for e in range(n):
            for l in range(spec.L):
                v[e * spec.n_params + spec.b[l]:e * spec.n_params + spec.b[l] + spec.dims[l + 1]] += np.float32(dense_bias)
    pst, qst = ps.fresh_stats(), np.concatenate([qs.fresh_stats() for _ in range(E)])
    if stats_away:
        kinds = ((0.3, 1.5), (0.2, 30.0), (-0.2, 0.02), (8.0, 1.2), (-8.0, 0.8))          # (running mean in deviations, running variance)
        for spec, v, n in ((ps, pst, 1), (qs, qst, E)):
            for e in range(n):
                for l in range(spec.L + 1):
                    D, o = spec.dims[l], e * spec.n_stats + spec.st[l]
                    if l == 0:
                        k = np.array([kinds[(c + e) % 5] for c in range(D)])
                        v[o:o + D], v[o + D:o + 2 * D] = k[:, 0] * np.sqrt(k[:, 1]), k[:, 1]
                        par = pp if spec is ps else qp                             # a clipped d moves its column by d_max scales: small scales there
                        par[e * spec.n_params + spec.bn[0]:e * spec.n_params + spec.bn[0] + D][np.abs(k[:, 0]) > 5] *= np.float32(0.2)
                    else:
                        v[o:o + D] = dense_bias + 0.4 + rng.uniform(-0.3, 0.3, D)
                        v[o + D:o + 2 * D] = (0.34 if dense_bias < 1 else 1.0) * np.exp(rng.uniform(np.log(0.5), np.log(2.0), D))
    batch = (f(rng.standard_normal((B, O))), f(rng.standard_normal((B, O))), f(np.tanh(rng.standard_normal((B, A)))), f(rng.standard_normal(B)),
             f(rng.random(B) < 0.2))
    cbatch = None if Oc is None else (f(rng.standard_normal((B, Oc))), f(rng.standard_normal((B, Oc))))
    z = lambda n: np.zeros(n)
    state = dict(pp=pp.astype(np.float64), pm=z(ps.n_params), pv=z(ps.n_params), ps=f(pst).astype(np.float64), qp=qp.astype(np.float64),
                 qm=z(E * qs.n_params), qv=z(E * qs.n_params), qs=f(qst).astype(np.float64), la=np.array([np.float64(np.float32(-0.3))]),
                 am=z(1), av=z(1), q_count=0, pi_count=0)
    eps = (f(rng.standard_normal((B, A))), f(rng.standard_normal((B, A))))
    return dict(ps=ps, qs=qs, state=state, batch=batch, cbatch=cbatch, eps=eps, h=hparams(A, E, warmup))


def cast_state(st, dtype):
    return {k: (v.astype(dtype) if isinstance(v, np.ndarray) else v) for k, v in st.items()}
