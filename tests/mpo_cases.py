"""The cases of tests/golden/mpo_reference.npz as the twin and the library take them (shared by test_mpo_twin.py and
test_gpu_mpo.py)."""
import os

import numpy as np

import mpo_twin as tw

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpo_reference.npz")
CASE_KEYS = ("v_min", "v_max", "action_clipping", "policy_init_scale", "max_grad_norm", "init_log_eta", "init_log_alpha_stddev")


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

    def sampled(self, name):
        return self.z[self.k + name + "_idx"], self.z[self.k + name + "_val"], float(self.z[self.k + name + "_norm"])


def load(c):
    return FixtureCase(np.load(FIXTURE), c)


def n_cases():
    return int(np.load(FIXTURE)["n_cases"])
