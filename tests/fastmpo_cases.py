"""Shared pieces of the FastMPO GPU tests: seeded cases for the float64 twin (tests/fastmpo_twin.py), one rlx_fastmpo_update_f32 call on
device copies of a twin state, and the comparison at the project's bars: metrics 1e-5 of max(|value|, 1) --
the expected-q values with the floor max(|v_min|, |v_max|) / 10; vectors 1e-5 relative L2, second Adam moments 5e-5; the parameter
step 2e-4 where the gradient (the first moment) is not negligible; the duals per entry as MPO's test has them."""
import numpy as np
import torch

import fastmpo_twin as tw
from rlx_amd.hip import FastMpoHparams, fastmpo_desc
from rlx_amd.hip.lib import FASTMPO_RESCALING

STATE_KEYS = ("p", "pm", "pv", "tp", "q", "qm", "qv", "tq", "d", "dm", "dv")
UPDATED = (("p", 1e-5), ("pm", 1e-5), ("pv", 5e-5), ("tp", 1e-5), ("q", 1e-5), ("qm", 1e-5), ("qv", 5e-5), ("tq", 1e-5), ("d", 1e-5),
           ("dm", 1e-5), ("dv", 5e-5))
Q_METRICS = tuple(tw.METRICS.index(k) for k in ("q/q_mean", "q/q_max", "q/q_min", "q/improvement_q_mean"))


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _t(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(dev)


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


def hparams(h):
    hp = FastMpoHparams()
    for k in ("gamma", "v_min", "v_max", "max_grad_norm", "policy_weight_decay", "critic_weight_decay", "dual_weight_decay", "critic_tau",
              "policy_tau", "epsilon_non_parametric", "epsilon_parametric_mu", "epsilon_parametric_sigma", "epsilon_penalty",
              "policy_init_scale", "policy_min_scale", "float_epsilon", "min_log_temperature", "min_log_alpha"):
        setattr(hp, k, float(h[k]))
    hp.adam_b1, hp.adam_b2, hp.adam_eps = float(h["adam_beta1"]), float(h["adam_beta2"]), 1e-8
    hp.action_sampling_number, hp.action_clipping = int(h["action_sampling_number"]), int(bool(h["action_clipping"]))
    hp.action_rescaling = FASTMPO_RESCALING[h["action_rescaling"]]
    hp.clipped_double_q_learning = int(bool(h["clipped_double_q_learning"]))
    hp.nr_critic_updates_per_policy_update = int(h["nr_critic_updates_per_policy_update"])
    hp.nr_policy_updates_per_step = int(h["nr_policy_updates_per_step"])
    return hp


class Case:
    """a seeded twin state, P G batches and the injected draws.  Rewards are drawn so that targets reach both support edges."""

    def __init__(self, seed, kind="fastsac", E=2, O=10, A=5, NA=51, B=13, K=4, P=2, G=2, policy_hidden=(128, 64, 64),
                 critic_hidden=(128, 64, 64), reward_scale=None, policy_kind=None, **over):
        self.h = h = dict(tw.HP, action_sampling_number=K, nr_policy_updates_per_step=P, nr_critic_updates_per_policy_update=G, **over)
        self.kind, self.policy_kind, self.E, self.O, self.A, self.NA, self.B, self.K, self.P, self.G = kind, policy_kind or kind, E, O, A, NA, B, K, P, G
        self.LP = tw.policy_layout(self.policy_kind, O, A, policy_hidden)
        self.LQ = tw.critic_layout(kind, O, A, NA, critic_hidden)
        self.desc = fastmpo_desc(O, O, A, NA, E == 2, self.policy_kind, kind, policy_hidden, critic_hidden)
        rng = np.random.default_rng(seed)
        p, tp = tw.make_params(seed, self.LP), tw.make_params(seed + 1, self.LP)
        q = np.concatenate([tw.make_params(seed + 10 + e, self.LQ, head_std=1.0) for e in range(E)])
        tq = np.concatenate([tw.make_params(seed + 20 + e, self.LQ, head_std=1.0) for e in range(E)])
        nd = 2 * A + 2
        d = tw.init_duals(A, h)
        d[1:1 + A] += f32(rng.standard_normal(A))            # log_alpha_mean != log_alpha_stddev, entry by entry
        self.st = dict(p=p, pm=np.zeros(p.size), pv=np.zeros(p.size), tp=tp, q=q, qm=np.zeros(q.size), qv=np.zeros(q.size), tq=tq, d=f32(d),
                       dm=np.zeros(nd), dv=np.zeros(nd))
        U = P * G
        dones = (rng.random((U, B)) < 0.2).astype(np.float64)
        truncs = dones * (rng.random((U, B)) < 0.5)
        rs = reward_scale if reward_scale is not None else 0.4 * (h["v_max"] - h["v_min"])
        self.batches = (f32(rng.standard_normal((U, B, O))), f32(rng.standard_normal((U, B, O))), f32(rng.standard_normal((U, B, A)) * 0.8),
                        f32(rng.standard_normal((U, B)) * rs), dones, truncs, rng.integers(1, 4, (U, B)).astype(np.float64))
        self.eps = (f32(rng.standard_normal((U, K, B, A))), f32(rng.standard_normal((P, K, 2 * B, A))))
        self.lrs = (f32(h["critic_learning_rate"] * (1.0 - 0.01 * np.arange(U))), f32(h["policy_learning_rate"] * (1.0 - 0.02 * np.arange(P))),
                    f32(h["dual_learning_rate"] * (1.0 - 0.03 * np.arange(P))))

    def twin(self, st=None, counts=(0, 0, 0)):
        return tw.update(self.st if st is None else st, self.LP, self.LQ, self.E, self.batches, self.eps[0], self.eps[1], self.h, counts,
                         *self.lrs)


class Run:
    """one rlx_fastmpo_update_f32 call on device copies of a twin state"""

    def __init__(self, ctx, dev, case, st=None, counts=(0, 0, 0), inject=True, key=(3, 7), h=None, desc=None):
        st = case.st if st is None else st
        self.nets = tuple(_t(st[k], dev) for k in STATE_KEYS)
        self.met = torch.zeros(len(tw.METRICS), device=dev)
        b = tuple(_t(x, dev) for x in case.batches)
        self.eps = tuple(_t(x, dev) for x in case.eps) if inject else None      # kept alive: the library holds the pointers
        if inject:
            ctx.dbg_set_sac_noise(*self.eps)
        try:
            self.counts = ctx.fastmpo_update(desc or case.desc, self.nets, b, np.array(key, np.uint32), counts, *case.lrs,
                                             hparams(h or case.h), self.met)
        finally:
            ctx.dbg_set_sac_noise(None, None)
        torch.cuda.synchronize()
        self.out = dict(zip(STATE_KEYS, (x.cpu().numpy().astype(np.float64) for x in self.nets)))
        self.metrics = self.met.cpu().numpy().astype(np.float64)


def metric_gaps(got, ref, h):
    """|got - ref| / max(|ref|, floor) per metric"""
    floor = np.ones(len(tw.METRICS))
    floor[list(Q_METRICS)] = max(max(abs(h["v_min"]), abs(h["v_max"])) / 10.0, 1.0)
    return np.abs(got - ref) / np.maximum(np.abs(ref), floor)


def check_dual_step(got, new, old):
    """the duals' step per entry (log_alpha_stddev sits near 1000, where the vector's relative L2 cannot see the step): each entry
    within 4 float32 ulps plus 1e-3 of its own step"""
    new, old = np.asarray(new, np.float64), np.asarray(old, np.float64)
    bar = 4.0 * np.spacing(np.abs(new).astype(np.float32)).astype(np.float64) + 1e-3 * np.abs(new - old)
    bad = np.nonzero(np.abs(got - new) > bar)[0]
    assert not bad.size, [(int(i), got[i], new[i], old[i]) for i in bad]


def figures(r, new, met, h, old):
    """every measured gap of a Run against the twin (printed by the tests in front of their assertions)"""
    f = {"metrics": float(metric_gaps(r.metrics, met, h).max())}
    for k, _ in UPDATED:
        f[k] = float(_rel(r.out[k], new[k]))
    for k, mk in (("p", "pm"), ("q", "qm")):
        g = new[mk]
        sel = np.abs(g) > 1e-3 * np.sqrt(np.mean(g * g))
        f[k + "_sel"] = float(sel.mean())
        f[k + "_step"] = float(_rel((r.out[k] - f32(old[k]))[sel], (new[k] - old[k])[sel]))
    return f


def min_selected(case):
    """the share of a network's entries whose gradient must count as not negligible for the step check to mean something: 0.9, the
    project's figure -- 0.8 where a network is of the ReLU kind (units dead on every row of a small batch have no gradient at all)"""
    return 0.8 if "fasttd3" in (case.kind, case.policy_kind) else 0.9


def check_against_twin(r, new, met, counts, h, old, step_tol=2e-4, min_sel=0.9):
    """step_tol: the parameter-step bar; a case that needs more than 2e-4 says where its figure comes from"""
    f = figures(r, new, met, h, old)
    print("fastmpo gaps:", {k: f"{v:.2e}" for k, v in f.items()})
    assert r.counts == tuple(counts), (r.counts, counts)
    assert np.all(np.isfinite(r.metrics)), r.metrics
    gaps = metric_gaps(r.metrics, met, h)
    bad = [(i, tw.METRICS[i], r.metrics[i], met[i]) for i in range(len(tw.METRICS)) if not gaps[i] <= 1e-5]
    assert not bad, bad
    check_dual_step(r.out["d"], new["d"], old["d"])
    bad = [(k, f[k]) for k, tol in UPDATED if not f[k] < tol]
    assert not bad, bad
    for k in ("p", "q"):
        assert f[k + "_sel"] > min_sel and f[k + "_step"] < step_tol, (k, f)
