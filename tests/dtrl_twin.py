"""CPU twin of dtrl.hip (not a test): loss_fn of rl_x/algorithms/ppo_dtrl/flax_full_jit/ppo_dtrl.py:184-245 with the projections of
trust_region_layer.py, restated in torch (float64 by default) on the flat parameter layout of oracle/nets.py, and two epochs of
`update` around it with oracle/ppo.py's optimiser.  The covariance projection is a torch.autograd.Function whose backward is the
reference's hand-written rule (trust_region_layer.py:82-135), the clamp of d_cov_pred at 1e-20 per row included; its root is found
by bisection, not by the reference's L-BFGS.  The reference is JAX only: PARITY WITH IT IS UNPINNED, as for the other JAX-only
parts; what pins this file are the known answers of tests/test_dtrl_twin.py."""
import math

import numpy as np
import torch

from oracle import nets, ppo

METRICS = ("loss/policy_gradient_loss", "loss/critic_loss", "loss/entropy_loss", "loss/trust_region_loss", "policy_ratio/approx_kl",
           "policy_ratio/clip_fraction", "projection/eta_mu", "projection/eta_cov", "projection/unprojected_kl_mean",
           "projection/projected_kl_mean", "projection/unprojected_kl_cov", "projection/projected_kl_cov")
C_ENT = 0.5 * math.log(2.0 * math.pi * math.e)


def kl_cov(std, so):
    return 0.5 * (2.0 * (torch.log(so) - torch.log(std)) + (std / so) ** 2 - 1.0).sum(-1)


def _proj_cov(eta, std, so):
    return (eta + 1.0) / torch.clamp(eta / so ** 2 + 1.0 / std ** 2, min=1e-8)


class CovProj(torch.autograd.Function):
    """std [mb, A] (every row the same vector), so [A] -> (projected covariance [mb, A], eta); the backward rule runs per row"""
    last_d_cov_pred = None          # the rows' d_cov_pred in front of the clamp (the tests look at its sign margin)

    @staticmethod
    def forward(ctx, std, so, bound):
        s = std[0]
        # the root is found in double whatever the dtype, as k_dtrl_cov_proj finds it: a float32 KL near a distant bound is noise, and
        # where a float32 bisection ends differs from one CPU to the next (no change in float64: .double() is the identity there)
        s64, so64 = s.detach().double(), so.detach().double()
        f = lambda eta: kl_cov(torch.sqrt(_proj_cov(eta, s64, so64)), so64) - bound
        lo, hi = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
        while f(hi) > 0:
            lo, hi = hi, 2.0 * hi
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if f(mid) > 0:
                lo = mid
            else:
                hi = mid
        eta = (0.5 * (lo + hi)).to(s.dtype)
        pc = torch.clamp(_proj_cov(eta, s, so), min=1e-16)
        ctx.save_for_backward(s, so, pc, eta)
        return pc.expand_as(std).clone(), eta

    @staticmethod
    def backward(ctx, d_proj, _d_eta):
        s, so, pc, eta = ctx.saved_tensors
        eo = eta + 1.0
        base = 1.0 / so ** 2 - 1.0 / s ** 2
        f2 = pc * (1.0 - pc / so ** 2)
        sum_val = (f2 * base / eo).sum()
        c = -1.0 / (torch.sign(sum_val) * 1e-8 if abs(sum_val) < 1e-8 else sum_val + 1e-12)
        deta_dq = c * f2 if eta > 0 else torch.zeros_like(f2)
        d_q = -pc * d_proj * pc
        d_eta = (d_q * (base / (eo * eo))).sum(1, keepdim=True)
        d_cov_pred = -(d_eta * deta_dq + d_q / eo) / s ** 4
        CovProj.last_d_cov_pred = d_cov_pred.detach().clone()
        d_cov_pred = torch.clamp(torch.nan_to_num(d_cov_pred), min=1e-20)
        return 2.0 * s * d_cov_pred, None, None


def loss_and_grads(pspec, pparams, cspec, cparams, states, actions, old_means, old_logstd, logp_old, returns, adv, global_step, h,
                   dtype=torch.float64, cstates=None):
    """adv: the minibatch's advantages as stored (normalised here).  h: clip_range, entropy_coef, critic_coef, mean_bound, cov_bound,
    trust_region_coef, total_timesteps.  cstates: the critic's own observations [mb, cspec.in_dim] (hp->critic_states); None: the
    critic reads `states`.  -> (loss, metrics [12], policy grads, critic grads, info)"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    pp, cp = t(pparams).requires_grad_(True), t(cparams).requires_grad_(True)
    x, a, mo, ols, lpo, ret = (t(v) for v in (states, actions, old_means, old_logstd, logp_old, returns))
    adv = t(ppo.normalize_advantages(np.asarray(adv, np.float64)))
    xc = x if cstates is None else t(cstates)
    mb, A = a.shape
    m = nets.torch_forward(pspec, pp, x)
    ls = pp[pspec.logstd:pspec.logstd + A]
    std, so = torch.exp(ls), torch.exp(ols)
    beta = (ols + C_ENT).sum() * 0.5 ** (10.0 * global_step / h["total_timesteps"])
    # mean projection (trust_region_layer.py:164-195)
    maha = 0.5 * (((mo - m) / so) ** 2).sum(1)
    m_on = maha > h["mean_bound"]
    safe = torch.where(m_on, maha, torch.ones_like(maha))
    pm = torch.where(m_on[:, None], mo + (m - mo) * torch.sqrt(h["mean_bound"] / safe)[:, None], m)
    eta_mu = torch.where(m_on, torch.sqrt(safe / h["mean_bound"]) - 1.0, torch.zeros_like(maha))
    post_mean = 0.5 * (((mo - pm) / so) ** 2).sum(1).detach()
    # covariance projection (:198-213): one scalar problem, the same for every row
    kl_c = kl_cov(std, so)
    cov_on = bool(kl_c > h["cov_bound"])
    eta = torch.zeros((), dtype=dtype)
    ps = std.expand(mb, A)
    if cov_on:
        pc, eta = CovProj.apply(std.expand(mb, A), so, h["cov_bound"])
        ps = torch.sqrt(pc)
    post_cov = kl_cov(ps[0], so).detach()
    # entropy projection (:218-233)
    pls = torch.log(ps)
    H = (pls + C_ENT).sum(1)
    ent_on = bool(H[0] < beta)
    pls2 = pls + ((beta - H) / A)[:, None] if ent_on else pls
    # trust-region regression loss against the detached projection (ppo_dtrl.py:197-201)
    pmd, psd = pm.detach(), ps.detach()
    tr = 0.5 * (((pmd - m) / psd) ** 2).sum(1) + 0.5 * (2.0 * (torch.log(psd) - ls) + (std / psd) ** 2 - 1.0).sum(1)
    # surrogate (:203-220)
    s2 = torch.exp(pls2)
    logp = (-0.5 * ((a - pm) / s2) ** 2 - 0.5 * math.log(2.0 * math.pi) - pls2).sum(1)
    entropy = (pls2 + C_ENT).sum(1)
    logratio = logp - lpo
    ratio = torch.exp(logratio)
    pg = torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1 - h["clip_range"], 1 + h["clip_range"]))
    vl = 0.5 * (nets.torch_forward(cspec, cp, xc).reshape(-1) - ret) ** 2
    loss = (pg - h["entropy_coef"] * entropy + h["trust_region_coef"] * tr + h["critic_coef"] * vl).mean()
    CovProj.last_d_cov_pred = None
    loss.backward()
    rows = (pg, vl, entropy, tr, (ratio - 1) - logratio, (torch.abs(ratio - 1) > h["clip_range"]).to(dtype), eta_mu, eta.expand(mb), maha,
            post_mean, kl_c.expand(mb), post_cov.expand(mb))
    info = {"maha": maha.detach().numpy(), "kl_cov": float(kl_c.detach()), "H": float(H[0].detach()), "beta": float(beta), "cov_on": cov_on, "ent_on": ent_on,
            "d_cov_pred": None if CovProj.last_d_cov_pred is None else CovProj.last_d_cov_pred.numpy(), "logp": logp.detach().numpy()}
    return float(loss.detach()), np.array([float(r.detach().mean()) for r in rows]), pp.grad.numpy(), cp.grad.numpy(), info


def update(pstate, cstate, states, actions, old_means, old_logstd, logp_old, returns, adv, batch_indices, lrs, global_step, h, cstates=None):
    """minibatch_update over the rows batch_indices [steps, mb] (ppo_dtrl.py:269-299) with oracle/ppo.py's TrainState (optax's clip +
    adam) -> (metrics [steps, 14], every step's info)"""
    out, infos = [], []
    for idx, lr in zip(batch_indices, lrs):
        _, met, gp, gc, info = loss_and_grads(pstate.spec, pstate.params, cstate.spec, cstate.params, states[idx], actions[idx], old_means[idx],
                                           old_logstd, logp_old[idx], returns[idx], adv[idx], global_step, h,
                                           cstates=None if cstates is None else cstates[idx])
        pn = pstate.apply_gradients(gp, lr, h["max_grad_norm"])
        cn = cstate.apply_gradients(gc, lr, h["max_grad_norm"])
        out.append(np.concatenate([met, [pn, cn]]))
        infos.append(info)
    return np.array(out), infos


def case(seed, A, mb, mean_on, cov_on, ent_on, obs=7, hidden=(64, 64, 64), B=None, act=nets.ACT_ELU, ln_first=True, cobs=None,
         chidden=None, old_ls_mean=0.0, ls_offset=None, cov_ratio=None, mixed=False, logp="rollout", step=None, act_scale=1.0):
    """Inputs whose branches no rounding decides: every row's maha is mean_bound x 4 or / 4, kl_cov is cov_bound x 4 or / 4, and the
    entropy lies on its side of beta by the offset between the two logstd vectors (the tests assert the margins on the twin).
    The defaults are the 60 cases of test_gpu_dtrl.py, bit for bit.  Beyond them: act / ln_first of both nets; cobs: the critic reads
    observations of its own, [B, cobs] (c["cstates"]), through hidden layers chidden; old_ls_mean: the centre of the rollout logstd;
    ls_offset: policy logstd - rollout logstd (default -2.5 behind an active entropy projection, else -0.5); cov_ratio: kl_cov /
    cov_bound (default 4 or 1/4 by cov_on); mixed: every third row's maha is 4 mean_bound and the others' mean_bound / 4 (mean_on is
    then ignored: mean_bound is 0.01); logp "policy": old log-probs are the twin's log-prob of the projected policy + U(-0.05, 0.05),
    every fourth row moved by +-0.35 (alternating), so a quarter of the ratios lies well outside the clip range of 0.1; step: the
    fraction global_step / total_timesteps (default 0 behind an active entropy projection, else 1); act_scale: the stored actions
    lie act_scale rollout standard deviations from the rollout means."""
    rng = np.random.default_rng(seed)
    B = B or mb
    pspec = nets.MLPSpec(obs, hidden, A, act, ln_first, True)
    cspec = nets.MLPSpec(obs if cobs is None else cobs, hidden if chidden is None else chidden, 1, act, ln_first, False)
    pp, cp = rng.normal(0, 0.12, pspec.n_params), rng.normal(0, 0.12, cspec.n_params)
    old_ls = rng.normal(old_ls_mean, 0.1, A)
    pp[pspec.logstd:] = old_ls + ((-2.5 if ent_on else -0.5) if ls_offset is None else ls_offset) + 0.3 * rng.normal(0, 1, A)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    pp, cp, old_ls, x = f32(pp), f32(cp), f32(old_ls), f32(rng.normal(0, 1, (B, obs)))
    mean = nets.forward(pspec, pp, x)[0]
    u = rng.normal(0, 1, (B, A))
    u *= np.sqrt(2.0 * 0.01 / ((u / np.exp(old_ls)) ** 2).sum(1, keepdims=True))       # maha = 0.01 on every row
    if mixed:                                                                          # maha = 0.04, 0.0025, 0.0025, 0.04, ...
        u *= np.where(np.arange(B) % 3 == 0, 2.0, 0.5)[:, None]
    old_means = f32(mean + u)
    actions = f32(old_means + act_scale * np.exp(old_ls) * rng.normal(0, 1, (B, A)))
    logp_old = f32(ppo.gaussian_log_prob(actions, old_means, old_ls[None, :]) + 0.05 * rng.normal(0, 1, B))
    kl = float(kl_cov(torch.tensor(np.exp(pp[pspec.logstd:])), torch.tensor(np.exp(old_ls))))
    h = dict(clip_range=0.1, entropy_coef=0.01, critic_coef=1.0, max_grad_norm=5.0,
             mean_bound=0.01 if mixed else 0.01 * (0.25 if mean_on else 4.0),
             cov_bound=kl * (0.25 if cov_on else 4.0) if cov_ratio is None else kl / cov_ratio, trust_region_coef=0.1, total_timesteps=1000.0)
    c = dict(pspec=pspec, cspec=cspec, pp=pp, cp=cp, states=x, actions=actions, old_means=old_means, old_logstd=old_ls, logp_old=logp_old,
             returns=f32(rng.normal(0, 1, B)), adv=f32(rng.normal(0.3, 1.5, B)),
             global_step=(0.0 if ent_on else 1000.0) if step is None else 1000.0 * step, h=h, cstates=None)
    if cobs is not None:    # (a generator of its own: the draws above are those of the case without it)
        c["cstates"] = f32(np.random.default_rng([seed, 1]).normal(0, 1, (B, cobs)))
    if ent_on:
        # behind an active entropy projection the entropy bonus passes nothing to the covariance projection; a row whose ratio is
        # clipped would then hand it an exactly zero cotangent, which has no sign: every ratio stays inside the clip range here
        c["logp_old"] = f32(run_case(c)[4]["logp"] + rng.uniform(-0.05, 0.05, B))
    elif logp == "policy":
        far = 0.35 * (np.arange(B) % 4 == 0) * np.where(np.arange(B) // 4 % 2 == 0, 1.0, -1.0)
        c["logp_old"] = f32(run_case(c)[4]["logp"] + rng.uniform(-0.05, 0.05, B) + far)
    return c


def run_case(c, dtype=torch.float64):
    return loss_and_grads(c["pspec"], c["pp"], c["cspec"], c["cp"], c["states"], c["actions"], c["old_means"], c["old_logstd"], c["logp_old"],
                          c["returns"], c["adv"], c["global_step"], c["h"], dtype, cstates=c.get("cstates"))


def margins_ok(c, info, cov_margin=2.0):
    """the conditions of a case whose branches and clamp sides no rounding decides.  The entropy lies on its side of beta by at least
    half of |beta| (beta is negative where the rollout logstd is small)"""
    h = c["h"]
    r = info["maha"] / h["mean_bound"]
    rc = info["kl_cov"] / h["cov_bound"]
    ok = bool(np.all((r < 0.5) | (r > 2.0))) and not 1.0 / cov_margin <= rc <= cov_margin
    ok = ok and (info["H"] < info["beta"] - 0.5 * abs(info["beta"]) if info["ent_on"] else info["H"] > info["beta"] + 0.5 * abs(info["beta"]))
    d = info["d_cov_pred"]
    if d is None:
        return ok
    # A = 1: one bound fixes the one projected variance whatever std is, so d_cov_pred is zero but for the rule's 1e-12 guard and no
    # input gives it a sign; there the condition is that either side of the clamp moves d logstd by less than 1e-10
    return ok and bool(np.all(np.abs(d) <= 1e-10) if d.shape[1] == 1 else np.all(np.abs(d) >= 1e-12))
