"""Helpers shared by the REPPO GPU tests (test_gpu_reppo.py, test_gpu_reppo_shapes.py): a Case (shapes, float32-representable
parameters, a batch), the library's hyperparameter struct from a dict, the KL-bound placement that splits a case's rows between
both branches of the `where`, and the comparison helpers with their tolerances."""
import numpy as np
import torch

import reppo_twin as tw
from rlx_amd.hip import ReppoHparams, reppo_desc

HP = dict(gamma=0.99, gae_lambda=0.95, v_min=-10.0, v_max=10.0, kl_bound=0.1, policy_min_std=0.0, auxiliary_loss_coefficient=1.0,
          max_grad_norm=0.5, nr_kl_samples=4)


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _close(a, b, floor=1.0):
    """1e-5 relative (L2), with an absolute floor per element: expected values sum_j p_j z_j over centers of order 10 cancel to
    ~1e-6 at initialisation, where float32 leaves ~1e-7"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= 1e-5 * max(np.linalg.norm(b), floor * np.sqrt(b.size))


def value_floor(h):
    """_close's floor for value expectations over the centers of [v_min, v_max]: the float32 rounding of sum_j p_j z_j scales with
    the centers' magnitude, while the near-uniform softmax of an initial critic cancels the sum to ~0 whatever the range -- so the
    floor grows with max(|v_min|, |v_max|) / 10 (1 at the +-10 the floor was set for)"""
    return max(abs(h["v_min"]), abs(h["v_max"])) / 10.0


def _hp(h):
    hp = ReppoHparams()
    for k in ("gamma", "gae_lambda", "v_min", "v_max", "kl_bound", "target_entropy", "policy_min_std", "auxiliary_loss_coefficient",
              "max_grad_norm"):
        setattr(hp, k, float(h[k]))
    hp.adam_b1, hp.adam_b2, hp.adam_eps = 0.9, 0.999, 1e-8
    hp.nr_kl_samples = int(h["nr_kl_samples"])
    return hp


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


class Case:
    """shapes, parameters (float32-representable) and a batch; O full columns, the policy / critic see index subsets.  Targets
    are N(0, 3) scaled by v_max / 10; targets_beyond: N(0, 1.2 v_max) with the first four rows on +-v_max and past them (the
    critic loss clamps them to the support).  eps_old_scale: the old policy's injected noise times this (exact in float32)"""

    def __init__(self, seed, B, O=13, A=3, Hp=64, Hc=64, NB=21, old_seed=None, obs_scale=1.0, targets_beyond=False, eps_old_scale=1.0,
                 **hp):
        self.h = dict(HP, **hp)
        self.h["target_entropy"] = A * 0.5
        rng = np.random.default_rng(seed)
        self.pidx = np.sort(rng.choice(O, O - 2, replace=False)).astype(np.int32)
        self.cidx = np.arange(O, dtype=np.int32)[::-1].copy()
        self.O, self.A, self.Hp, self.Hc, self.NB, self.B = O, A, Hp, Hc, NB, B
        Op, Oc = len(self.pidx), len(self.cidx)
        self.desc = reppo_desc(Op, Oc, A, Hp, Hc, NB)
        self.LP, self.LQ = tw.policy_layout(Op, A, Hp), tw.critic_layout(Oc, A, Hc, NB)
        self.p, self.q = tw.make_params(seed, Op, Oc, A, Hp, Hc, NB, self.h["v_min"], self.h["v_max"], 0.05, 0.02)
        self.old_p = self.p if old_seed is None else tw.make_params(old_seed, Op, Oc, A, Hp, Hc, NB, self.h["v_min"], self.h["v_max"])[0]
        r32 = lambda *sh: _f32(rng.standard_normal(sh))
        self.states = _f32(r32(B, O) * obs_scale)
        self.actions = _f32(np.tanh(r32(B, A)))
        self.rewards = _f32(r32(B) * 2.0)
        self.targets = _f32(r32(B) * 3.0 * (self.h["v_max"] / 10.0))
        self.next_features = rng.standard_normal((B, Hc), dtype=np.float32) * np.float32(0.5)
        self.terms = (rng.random(B) < 0.2).astype(np.float64)
        self.truncs = ((rng.random(B) < 0.15) & (self.terms == 0)).astype(np.float64)
        self.eps_new = r32(B, A)
        self.eps_old = r32(self.h["nr_kl_samples"], B, A) * eps_old_scale
        if targets_beyond:
            v = self.h["v_max"]
            self.targets = _f32(r32(B) * 1.2 * v)
            self.targets[:4] = [v, self.h["v_min"], 2.5 * v, -1.375 * v]
            self.truncs[:4] = 0.0          # their cross-entropy terms count

    def batch_twin(self):
        return (self.states[:, self.cidx], self.actions, self.targets, self.rewards, self.next_features, self.terms, self.truncs)

    def batch_dev(self, dev):
        return tuple(_t(x, dev) for x in (self.states, self.actions, self.rewards, self.targets, self.next_features, self.terms, self.truncs))


def place_kl_bound(c):
    """an old policy that differs: put the bound between two rows' KL values near the median, far from every row"""
    if c.old_p is not c.p:
        kl = tw.policy_loss(torch.tensor(c.p, dtype=torch.float64), c.LP, c.old_p, c.q, c.LQ, c.states[:, c.pidx], c.states[:, c.cidx],
                            tw._t(c.eps_new), tw._t(c.eps_old), c.h)[2]
        s = np.sort(kl)
        mid = len(s) // 2
        i = max(range(mid - len(s) // 4, mid + len(s) // 4), key=lambda j: s[j + 1] - s[j])
        c.h["kl_bound"] = float(np.float32(0.5 * (s[i] + s[i + 1])))
        assert (s[i + 1] - s[i]) / 2 > 1e-4      # every row's KL at least 1e-4 from the bound: far beyond float32 error
    return c


def _with_noise(ctx, eps_next, eps_cur, fn):
    ctx.dbg_set_sac_noise(eps_next, eps_cur)
    try:
        return fn()
    finally:
        ctx.dbg_set_sac_noise(None, None)
