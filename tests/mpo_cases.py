"""The cases of tests/golden/mpo_reference.npz as the twin and the library take them, and the helpers shared by the MPO tests
(test_mpo_twin.py, test_gpu_mpo.py, test_gpu_mpo_shapes.py): the library's hyperparameter struct from a dict, one
rlx_mpo_update_f32 call on device copies of a twin state, and the comparisons with their tolerances -- 1e-5 relative (L2 per
vector); second Adam moments 5e-5 (float32's 1 - b2); the expected-q metric with a floor of max|v| / 10 (its value is a difference
of atoms that large)."""
import os

import numpy as np
import torch

import mpo_twin as tw
from rlx_amd.hip import MpoHparams

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpo_reference.npz")
CASE_KEYS = ("v_min", "v_max", "action_clipping", "policy_init_scale", "max_grad_norm", "init_log_eta", "init_log_alpha_stddev")
STATE_KEYS = ("p", "pm", "pv", "tp", "q", "qm", "qv", "tq", "d", "dm", "dv")
# (state key, bar): the vectors an update writes
UPDATED = (("p", 1e-5), ("pm", 1e-5), ("pv", 5e-5), ("q", 1e-5), ("qm", 1e-5), ("qv", 5e-5), ("d", 1e-5), ("dm", 1e-5), ("dv", 5e-5))


class SecondCall:
    """the fixture's second `update` of a case (step 2, the reference's Adam state carried over from the first call): its noise
    and outputs; the sampled networks sit at the first call's positions"""

    def __init__(self, z, k):
        self.z, self.k, self.u = z, k, k + "u2_"
        self.eps_c, self.eps_a = z[self.u + "eps_c"], z[self.u + "eps_a"]
        self.metrics = z[self.u + "metrics"]
        self.duals, self.dm, self.dv = (z[self.u + n] for n in ("duals_after", "duals_exp_avg", "duals_exp_avg_sq"))

    def sampled(self, name):
        return self.z[self.k + name + "_idx"], self.z[self.u + name + "_val"], float(self.z[self.u + name + "_norm"])


class FixtureCase:
    def __init__(self, z, c):
        k = "c%d_" % c
        self.k, self.z = k, z
        g = lambda n: z[k + n]
        self.O, self.A, self.H, self.NA, self.B, self.S = (int(g(n)) for n in ("obs_dim", "act_dim", "hidden", "nr_atoms", "batch", "S"))
        self.pidx, self.cidx = g("pidx"), g("cidx")
        self.Op, self.Oc = len(self.pidx), len(self.cidx)
        self.h = dict(tw.HP, action_sampling_number=self.S, **{n: g(n).item() for n in CASE_KEYS})
        self.h["action_clipping"] = bool(self.h["action_clipping"])
        self.LP, self.LQ = tw.policy_layout(self.Op, self.A, self.H), tw.critic_layout(self.Oc, self.A, self.H, self.NA)
        p, q = tw.make_params(int(g("param_seed")), self.Op, self.Oc, self.A, self.H, self.NA)
        ts = int(g("target_seed"))
        tp, tq = (p, q) if ts < 0 else tw.make_params(ts, self.Op, self.Oc, self.A, self.H, self.NA)
        zp, zq, nd = np.zeros(p.size), np.zeros(q.size), 2 * self.A + 2
        self.state = dict(p=p, pm=zp, pv=zp, tp=tp, q=q, qm=zq, qv=zq, tq=tq, d=g("duals0"), dm=np.zeros(nd), dv=np.zeros(nd))
        self.batch = tuple(g(n) for n in ("states", "next_states", "actions", "rewards", "dones", "truncs", "nsteps"))
        self.eps_c, self.eps_a, self.eps_act = g("eps_c"), g("eps_a"), g("eps_act")
        self.low, self.high = g("low"), g("high")
        self.full_obs = self.Op != self.O or self.Oc != self.O
        self.second = SecondCall(z, k) if k + "u2_metrics" in z.files else None

    def sampled(self, name):
        return self.z[self.k + name + "_idx"], self.z[self.k + name + "_val"], float(self.z[self.k + name + "_norm"])

    def indices(self):
        return (self.pidx, self.cidx) if self.full_obs else (None, None)


def load(c):
    return FixtureCase(np.load(FIXTURE), c)


def n_cases():
    return int(np.load(FIXTURE)["n_cases"])


def two_call_cases():
    z = np.load(FIXTURE)
    return [c for c in range(int(z["n_cases"])) if "c%d_u2_metrics" % c in z.files]


def _t(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(dev)


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


def _hp(h):
    hp = MpoHparams()
    for k in ("gamma", "v_min", "v_max", "max_grad_norm", "epsilon_non_parametric", "epsilon_parametric_mu", "epsilon_parametric_sigma",
              "epsilon_penalty", "policy_init_scale", "policy_min_scale", "float_epsilon", "min_log_temperature", "min_log_alpha"):
        setattr(hp, k, float(h[k]))
    hp.adam_b1, hp.adam_b2, hp.adam_eps = 0.9, 0.999, 1e-8
    hp.action_sampling_number, hp.action_clipping, hp.action_rescaling = int(h["action_sampling_number"]), int(bool(h["action_clipping"])), int(bool(h["action_rescaling"]))
    return hp


class Run:
    """one rlx_mpo_update_f32 call on device copies of a twin state"""

    def __init__(self, ctx, dev, desc, st, batch, hp_dict, eps=None, pidx=None, cidx=None, key=(0, 7), step=1):
        self.nets = tuple(_t(st[k], dev) for k in STATE_KEYS)
        self.met = torch.zeros(17, device=dev)
        hp = _hp(hp_dict)
        b = tuple(_t(x, dev) for x in batch)
        pi = None if pidx is None else _t(pidx, dev, np.int32)
        ci = None if cidx is None else _t(cidx, dev, np.int32)
        self.eps = None if eps is None else (_t(eps[0], dev), _t(eps[1], dev))     # kept alive: the library holds the pointers
        if eps is not None:
            ctx.dbg_set_sac_noise(*self.eps)
        try:
            self.key = ctx.mpo_update(desc, self.nets, b, np.array(key, np.uint32), step, hp_dict["agent_learning_rate"],
                                      hp_dict["dual_learning_rate"], hp, self.met, pidx=pi, cidx=ci)
        finally:
            ctx.dbg_set_sac_noise(None, None)
        torch.cuda.synchronize()
        self.out = dict(zip(STATE_KEYS, (x.cpu().numpy().astype(np.float64) for x in self.nets)))
        self.metrics = self.met.cpu().numpy().astype(np.float64)


def _check_metrics(got, ref, vmax):
    floor = np.ones(17)
    floor[5] = max(vmax / 10.0, 1.0)
    bad = [(i, tw.METRICS[i], got[i], ref[i]) for i in range(17) if abs(got[i] - ref[i]) > 1e-5 * max(abs(ref[i]), floor[i])]
    assert not bad, bad


def check_dual_step(got, new, old):
    """the duals' step per entry: log_alpha_stddev sits near 1000, where the whole vector's relative L2 cannot see the step
    (~1e-2); each entry within 4 float32 ulps plus 1e-3 of its own step"""
    new, old = np.asarray(new, np.float64), np.asarray(old, np.float64)
    bar = 4.0 * np.spacing(np.abs(new).astype(np.float32)).astype(np.float64) + 1e-3 * np.abs(new - old)
    bad = np.nonzero(np.abs(got - new) > bar)[0]
    assert not bad.size, [(int(i), got[i], new[i], old[i]) for i in bad]


def check_against_twin(r, new, met, h, old=None):
    """a Run against the twin's update: the 17 metrics and all 11 state vectors (the targets bit for bit: read only); with the
    state before the update, the duals' step per entry"""
    _check_metrics(r.metrics, met, max(abs(h["v_min"]), abs(h["v_max"])))
    if old is not None:
        check_dual_step(r.out["d"], new["d"], old["d"])
    bad = [(k, _rel(r.out[k], new[k])) for k, tol in UPDATED if not _rel(r.out[k], new[k]) < tol]
    assert not bad, bad
    for k in ("tp", "tq"):
        assert np.array_equal(r.out[k], np.asarray(new[k], np.float32).astype(np.float64)), k
