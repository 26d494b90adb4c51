"""CPU twin (test infrastructure) of droq.hip: the reference's DroQ `update` restated in numpy, written from
rl_x/algorithms/droq/flax/droq.py:144-261 and critic.py:17-35.  DroQ is REDQ (tests/redq_twin.py, whose loss heads, state layout and
input recipe are used here) with other critics:

  critic block   critic.py:27-30, :31-34   Dense -> Dropout -> LayerNorm (flax: eps 1e-6, scale, bias, "fast variance") -> ReLU in
                                           EVERY hidden block; dropout active in every pass (deterministic=False)
  critic step i  droq.py:228-242           redq.py's, the online critics and the selected targets each under their own masks
  policy step    droq.py:246-253           redq.py's, the E critics on (s_0, a~) under a third set of masks

The noise, the subsets AND THE MASKS are inputs.  The masks of the library are its own documented stream (include/rlx_hip.h,
DESIGN.md 4.5g); mask_stream below restates it from oracle/prng.py's split, random_bits and uniform alone, one row at a time, and
mask_rows is the same stream for all rows at once (the partitionable scheme's block function, tests/test_droq_twin.py holds the two
equal).  The reference's DroQ exists in JAX only and JAX is not installed: PARITY UNPINNED by the reference; tests/test_droq_twin.py
pins the twin with hand-computed answers and float64 torch.autograd.

FLAT LAYOUT of one critic: per hidden block W[in, out], b[out], LN scale[out], LN bias[out]; then the head W[in, 1], b[1]; E critics
back to back.  Q matrices here are [B, E]; the library's are [E, B].  The dtype of the state is the dtype of the whole evaluation."""
import numpy as np

import redq_twin as rt
from oracle import nets, prng, sac

METRICS = rt.METRICS
STATE_KEYS = rt.STATE_KEYS
LN_EPS = 1e-6

# where row b's keys sit in a step's split (droq.py:229-230, :247-248): (base, stride, count) with count = 3 B + 2 / 2 B + 1
LAYOUTS = {"next_noise": lambda B: (2, 3, 3 * B + 2), "online": lambda B: (3, 3, 3 * B + 2), "target": lambda B: (4, 3, 3 * B + 2),
           "cur_noise": lambda B: (1, 2, 2 * B + 1), "policy": lambda B: (2, 2, 2 * B + 1)}


# ------------------------------------------------------------------------------------------------------------ the mask stream
def keep_prob(rate):
    """keep = 1 - rate in float32, as the library forms it"""
    return np.float32(1.0) - np.float32(rate)


def mask_stream(step_key, layout, j, E, l, L, B, D, rate, partitionable=True):
    """-> bool [B, D]: unit u of row b is kept iff uniform(layer_key, (D,))[u] < keep, layer_key = split(split(split(step_key,
    count)[base + stride b], E)[j], L)[l].  Only oracle.prng's split, random_bits (inside uniform) and uniform."""
    base, stride, count = layout
    rows = prng.split(step_key, count, partitionable)
    out = np.ones((B, D), bool)
    if rate == 0:
        return out
    for b in range(B):
        net_key = prng.split(rows[base + stride * b], E, partitionable)[j]
        layer_key = prng.split(net_key, L, partitionable)[l]
        out[b] = prng.uniform(layer_key, (D,), partitionable=partitionable) < keep_prob(rate)
    return out


def mask_rows(step_key, layout, j, E, l, L, B, D, rate):
    """mask_stream under the partitionable scheme for all rows at once: split(key, n)[i] = threefry(key, (0, i)) and
    random_bits(key, (D,))[u] = the xor of threefry(key, (0, u))'s two words (oracle/prng.py)"""
    base, stride, count = layout
    if rate == 0:
        return np.ones((B, D), bool)
    rows = prng.split(step_key, count, True)[base:base + stride * B:stride]
    n0, n1 = prng.threefry2x32(rows[:, 0], rows[:, 1], 0, j)
    k0, k1 = prng.threefry2x32(n0, n1, 0, l)
    b0, b1 = prng.threefry2x32(k0[:, None], k1[:, None], 0, np.arange(D, dtype=np.uint32)[None])
    return prng._bits_to_unit_float(b0 ^ b1) < keep_prob(rate)


def update_masks(step_keys, B, hidden, E, M, rate, partitionable=True, fast=False):
    """every mask of one update from the key each step splits (step_keys: G + 1 keys) -> {"online": [G][E][L], "target": [G][M][L],
    "policy": [E][L]} of bool [B, D_l]"""
    L, G = len(hidden), len(step_keys) - 1
    one = (lambda k, lay, j, l: mask_rows(k, lay, j, E, l, L, B, hidden[l], rate)) if fast and partitionable else \
        (lambda k, lay, j, l: mask_stream(k, lay, j, E, l, L, B, hidden[l], rate, partitionable))
    nets_ = lambda k, lay, n: [[one(k, lay, j, l) for l in range(L)] for j in range(n)]
    return {"online": [nets_(step_keys[i], LAYOUTS["online"](B), E) for i in range(G)],
            "target": [nets_(step_keys[i], LAYOUTS["target"](B), M) for i in range(G)],
            "policy": nets_(step_keys[G], LAYOUTS["policy"](B), E)}


def swap_online_target(masks, M):
    """the masks with the online and target streams exchanged (networks 0 .. M - 1; what reading the wrong key layout would give)"""
    G = len(masks["online"])
    online = [[masks["target"][i][e] if e < M else masks["online"][i][e] for e in range(len(masks["online"][i]))] for i in range(G)]
    return {"online": online, "target": [masks["online"][i][:M] for i in range(G)], "policy": masks["policy"]}


# ------------------------------------------------------------------------------------------------------------ the critic
class CriticSpec:
    """offsets of one critic in the flat vector (layout above)"""

    def __init__(self, in_dim, hidden, out_dim=1):
        self.in_dim, self.hidden, self.out_dim = int(in_dim), [int(h) for h in hidden], int(out_dim)
        off, d, self.layers = 0, self.in_dim, []
        for h in self.hidden:
            L = {"in": d, "out": h, "W": off, "b": off + d * h, "g": off + d * h + h, "be": off + d * h + 2 * h}
            off += d * h + 3 * h
            self.layers.append(L)
            d = h
        self.head = {"in": d, "out": self.out_dim, "W": off, "b": off + d * self.out_dim}
        self.n_params = off + d * self.out_dim + self.out_dim


def block_forward(z, mask, keep, g, be):
    """critic.py:28-30: z [B, D] (the Dense output) -> (relu(LN(z') g + be), cache), z' = mask ? z / keep : 0"""
    dt = z.dtype
    zd = np.where(mask, z / dt.type(keep), dt.type(0)).astype(dt)
    mu = zd.mean(axis=1, keepdims=True)
    var = np.maximum(0, (zd * zd).mean(axis=1, keepdims=True) - mu * mu)
    rstd = (1.0 / np.sqrt(var + dt.type(LN_EPS))).astype(dt)
    xhat = ((zd - mu) * rstd).astype(dt)
    h = np.maximum(xhat * g + be, 0).astype(dt)
    return h, {"mask": mask, "keep": dt.type(keep), "zd": zd, "mu": mu, "rstd": rstd, "xhat": xhat, "h": h, "g": g}


def block_backward(dh, c):
    """-> (dz [B, D], d scale [D], d bias [D]): dz = (mask / keep) LNbwd(dh relu')"""
    dt = dh.dtype
    d = (dh * (c["h"] > 0)).astype(dt)
    dxh = d * c["g"]
    m1 = dxh.mean(axis=1, keepdims=True)
    m2 = (dxh * c["xhat"]).mean(axis=1, keepdims=True)
    dzd = c["rstd"] * (dxh - m1 - c["xhat"] * m2)
    dz = np.where(c["mask"], dzd / c["keep"], dt.type(0)).astype(dt)
    return dz, (d * c["xhat"]).sum(axis=0).astype(dt), d.sum(axis=0).astype(dt)


def _mat(p, L):
    return p[L["W"]:L["W"] + L["in"] * L["out"]].reshape(L["in"], L["out"])


def critic_forward(qs, p, x, masks, keep):
    """one critic on x [B, in] under masks [L] of [B, D_l] -> (q [B, 1], cache)"""
    dt = p.dtype
    h = x.astype(dt)
    cache = {"x": h, "blocks": []}
    for L, m in zip(qs.layers, masks):
        z = (h @ _mat(p, L) + p[L["b"]:L["b"] + L["out"]]).astype(dt)
        h, c = block_forward(z, m, keep, p[L["g"]:L["g"] + L["out"]], p[L["be"]:L["be"] + L["out"]])
        cache["blocks"].append(c)
    H = qs.head
    return (h @ _mat(p, H) + p[H["b"]:H["b"] + H["out"]]).astype(dt), cache


def critic_backward(qs, p, cache, d_out, need_dx=False):
    """the reverse pass of critic_forward -> flat gradient (and d / dx)"""
    dt = p.dtype
    g = np.zeros(qs.n_params, dt)
    H, blocks = qs.head, cache["blocks"]
    g[H["W"]:H["W"] + H["in"] * H["out"]] = (blocks[-1]["h"].T @ d_out).ravel()
    g[H["b"]:H["b"] + H["out"]] = d_out.sum(axis=0)
    dh = d_out @ _mat(p, H).T
    dx = None
    for li in range(len(qs.layers) - 1, -1, -1):
        L = qs.layers[li]
        dz, dg, db = block_backward(dh.astype(dt), blocks[li])
        g[L["g"]:L["g"] + L["out"]], g[L["be"]:L["be"] + L["out"]] = dg, db
        inp = cache["x"] if li == 0 else blocks[li - 1]["h"]
        g[L["W"]:L["W"] + L["in"] * L["out"]] = (inp.T @ dz).ravel()
        g[L["b"]:L["b"] + L["out"]] = dz.sum(axis=0)
        if li > 0 or need_dx:
            dh = dz @ _mat(p, L).T
            dx = dh if li == 0 else dx
    return (g, dx) if need_dx else g


def lecun_ln_init(qs, rng):
    """flax defaults: lecun_normal kernels, zero biases, LayerNorm scale 1 and bias 0"""
    plain = nets.MLPSpec(qs.in_dim, qs.hidden, qs.out_dim, nets.ACT_RELU, False, False)
    flat, p = sac.lecun_normal_init(plain, rng), np.zeros(qs.n_params)
    for L, Lp in zip(qs.layers + [qs.head], plain.layers + [plain.head]):
        n = L["in"] * L["out"] + L["out"]
        p[L["W"]:L["W"] + n] = flat[Lp["W"]:Lp["W"] + n]
        if "g" in L:
            p[L["g"]:L["g"] + L["out"]] = 1.0
    return p


# ------------------------------------------------------------------------------------------------------------ the update
def problem(seed, O, A, B, ph, qh, E, M, G, Oc=None, rate=0.0):
    """tests/redq_twin.py's input recipe with DroQ's critics (init + 0.02 noise on EVERY entry, LayerNorm parameters included, so
    that no scale is exactly 1 and no bias exactly 0) -> dict(ps, qs, state (float64), batch, cbatch or None, h)"""
    p = rt.problem(seed, O, A, B, ph, qh, E, M, G, Oc)
    p["h"]["dropout_rate"] = float(rate)
    rng = np.random.default_rng(seed + 77)
    qs = CriticSpec((O if Oc is None else Oc) + A, qh, 1)
    qp = (np.concatenate([lecun_ln_init(qs, rng) for _ in range(E)]) + 0.02 * rng.standard_normal(E * qs.n_params)).astype(np.float32)
    qtp = (qp + 0.01 * rng.standard_normal(qp.shape)).astype(np.float32)
    p["qs"], p["state"] = qs, rt.zero_state(p["state"]["P"], qp, qtp, np.float32(-0.3))
    return p


def critic_step(ps, qs, pp, qp, qtp, log_alpha, batch, eps1, subset, m_online, m_target, h, cs=None, cs2=None):
    """critic_loss_fn meaned (droq.py:148-176, :217-222) -> (q_loss, gcritic [E n], y [B]); m_online [E][L], m_target [M][L]: the
    m-th SELECTED target runs under m_target[m]"""
    s, s2, a, r, term = batch
    cs = s if cs is None else cs
    cs2 = s2 if cs2 is None else cs2
    dt = qp.dtype
    E, n, keep = int(h["ensemble_size"]), qs.n_params, keep_prob(h["dropout_rate"])
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    nm, nls, _, _ = sac.policy_forward(ps, pp, s2, lo, hi)
    na, nlogp = sac.tanh_gaussian(nm, nls, eps1)
    x2 = np.concatenate([cs2, na], axis=1)
    qn = np.concatenate([critic_forward(qs, qtp[t * n:(t + 1) * n], x2, m_target[m], keep)[0] for m, t in enumerate(subset)], axis=1)
    x = np.concatenate([cs, a], axis=1)
    outs, caches = zip(*(critic_forward(qs, qp[e * n:(e + 1) * n], x, m_online[e], keep) for e in range(E)))
    y, loss, dq = rt.critic_loss(np.concatenate(outs, axis=1), qn, r, term, alpha, nlogp, dt.type(h["gamma"]))
    g = np.concatenate([critic_backward(qs, qp[e * n:(e + 1) * n], caches[e], dq[:, e:e + 1].astype(dt)) for e in range(E)])
    return loss.mean(), g, y


def policy_step(ps, qs, pp, qp, log_alpha, s, eps2, m_policy, h, cs=None):
    """policy_entropy_loss_fn meaned (droq.py:179-215) -> (metrics, gpolicy, g_log_alpha); m_policy [E][L]"""
    cs = s if cs is None else cs
    dt = pp.dtype
    B = s.shape[0]
    E, n, keep = int(h["ensemble_size"]), qs.n_params, keep_prob(h["dropout_rate"])
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    alpha = np.exp(log_alpha)
    cm, cls, cls_raw, pc = sac.policy_forward(ps, pp, s, lo, hi)
    std = np.exp(cls)
    ca, clogp = sac.tanh_gaussian(cm, cls, eps2)
    entropy = -clogp
    x = np.concatenate([cs, ca], axis=1)
    outs, caches = zip(*(critic_forward(qs, qp[e * n:(e + 1) * n], x, m_policy[e], keep) for e in range(E)))
    min_q, seed = rt.policy_seed(np.concatenate(outs, axis=1))
    Oc = cs.shape[1]
    dq_da = np.zeros_like(ca)
    for e in range(E):
        _, dx = critic_backward(qs, qp[e * n:(e + 1) * n], caches[e], seed[:, e:e + 1].astype(dt), need_dx=True)
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


def update(ps, qs, st, batch, eps1, eps2, subsets, masks, h, *rates_and_critic_states):
    """`update` (droq.py:144-261): tests/redq_twin.py's run_update over this file's steps, with the target subsets [G, M] and the
    masks (update_masks' structure) as two more inputs"""
    return rt.run_update(lambda i, P, Q, QT, la, b, e1, cs, cs2: critic_step(ps, qs, P, Q, QT, la, b, e1, list(subsets[i]), masks["online"][i],
                                                                             masks["target"][i], h, cs, cs2),
                         lambda P, Q, la, s, e2, cs: policy_step(ps, qs, P, Q, la, s, e2, masks["policy"], h, cs),
                         st, batch, eps1, eps2, h, *rates_and_critic_states)


def losses_torch(ps, pp, qs, qp, qtp, log_alpha, batch, eps1, eps2, subset, m_online, m_target, m_policy, h, critic_states=None,
                 critic_next_states=None):
    """ONE critic step's loss and the policy / entropy loss on the same parameters, restated with torch ops (float64, the masks as
    constants, torch.nn.functional.layer_norm) and differentiated by torch.autograd -> (q_loss, gQ, policy + entropy loss, gP, gLA)"""
    import torch
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    P, Q, LA = t(pp).requires_grad_(True), t(qp).requires_grad_(True), t(log_alpha).requires_grad_(True)
    QT = t(qtp)
    A = ps.out_dim // 2
    E, n, keep = int(h["ensemble_size"]), qs.n_params, float(keep_prob(h["dropout_rate"]))
    lo, hi = h.get("log_std_min", -20.0), h.get("log_std_max", 2.0)
    s, s2, a, r, term = (t(x) for x in batch)
    cs = s if critic_states is None else t(critic_states)
    cs2 = s2 if critic_next_states is None else t(critic_next_states)

    def pol(params, x):
        out = nets.torch_forward(ps, params, x)
        return out[:, :A], torch.clamp(out[:, A:], lo, hi)

    def critic(p, x, masks):
        hcur = x
        for L, m in zip(qs.layers, masks):
            z = hcur @ p[L["W"]:L["W"] + L["in"] * L["out"]].view(L["in"], L["out"]) + p[L["b"]:L["b"] + L["out"]]
            z = torch.where(torch.tensor(np.asarray(m)), z / keep, torch.zeros_like(z))
            hcur = torch.relu(torch.nn.functional.layer_norm(z, (L["out"],), p[L["g"]:L["g"] + L["out"]], p[L["be"]:L["be"] + L["out"]], LN_EPS))
        H = qs.head
        return hcur @ p[H["W"]:H["W"] + H["in"] * H["out"]].view(H["in"], H["out"]) + p[H["b"]:H["b"] + H["out"]]

    def qvals(params, which, masks, obs, act):
        x = torch.cat([obs, act], dim=1)
        return torch.cat([critic(params[e * n:(e + 1) * n], x, masks[k]) for k, e in enumerate(which)], dim=1)

    def tg(mean, ls, eps):
        u = mean + torch.exp(ls) * eps
        act = torch.tanh(u)
        return act, (-0.5 * ((u - mean) / torch.exp(ls)) ** 2 - 0.5 * rt.tt.LOG_2PI - ls - torch.log(1.0 - act ** 2 + 1e-6)).sum(1)

    alpha_g = torch.exp(LA)
    alpha = alpha_g.detach()
    na, nlp = tg(*pol(P.detach(), s2), t(eps1))
    y = r + h["gamma"] * (1 - term) * (qvals(QT, list(subset), m_target, cs2, na).min(dim=1).values - alpha * nlp)
    q_loss = ((qvals(Q, range(E), m_online, cs, a) - y[:, None]) ** 2).mean()
    gQ, = torch.autograd.grad(q_loss, Q)
    ca, clp = tg(*pol(P, s), t(eps2))
    entropy = (-clp).detach()
    min_q = qvals(Q.detach(), range(E), m_policy, cs, ca).min(dim=1).values
    pe_loss = (alpha * clp - min_q + alpha_g * (entropy - h["target_entropy"])).mean()
    gP, gLA = torch.autograd.grad(pe_loss, (P, LA))
    return q_loss.item(), gQ.numpy(), pe_loss.item(), gP.numpy(), gLA.item()
