"""Helpers shared by the TD3 / DDPG tests (test_td3_cases.py on the CPU, test_gpu_td3.py on the GPU): the case table of
rlx_td3_update_f32, the figures a run is judged by, and the perturbed twins -- the faults the bars have to see.

| case          | seed | O / Oc  | A  | policy hidden | critic hidden | E | B    | what it runs                                             |
|---------------|------|---------|----|---------------|---------------|---|------|----------------------------------------------------------|
| critic_only   | 511  | 5 / 5   | 2  | (64, 64)      | (64, 64)      | 2 | 67   | policy_step = 0: targets and policy unchanged            |
| full          | 511  | 5 / 5   | 2  | (64, 64)      | (64, 64)      | 2 | 67   | the critic and the policy step                           |
| ddpg          | 512  | 5 / 5   | 2  | (64, 64)      | (64, 64)      | 1 | 67   | nr_critics = 1, joint                                    |
| two_calls     | 511  | 5 / 5   | 2  | (64, 64)      | (64, 64)      | 2 | 67   | a critic-only call, then a full one at annealed rates    |
| critic_states | 513  | 12 / 9  | 3  | (64, 64)      | (64, 64)      | 2 | 70   | the critics' own observation columns                     |
| narrow        | 514  | 5 / 5   | 1  | (64)          | (64)          | 2 | 1    | one row, one action dimension, one hidden layer          |
| act64         | 515  | 70 / 29 | 64 | (128, 64, 64) | (128, 64, 64) | 2 | 37   | the widest action, three hidden layers                   |
| split_ragged  | 516  | 45 / 45 | 17 | (256, 128)    | (256, 128)    | 2 | 4099 | the split-operand engine (>= 4096 rows), a ragged tail   |

The inputs are drawn from the seed (td3_twin.problem), the injected noise from seed + 1.  tests/test_td3_cases.py holds every case
to the envelope, to half of its bar between the float32 and the float64 twin, and to |Q1 - Q2| > 2e-5 on the policy step's rows."""
import numpy as np

import td3_twin as tw
from oracle import nets

GAMMA, TAU, LR = 0.99, 0.005, 3e-4
LR2 = (2.7e-4, 2.4e-4)          # (policy, critics) of two_calls' second call: linear_schedule at unequal counts (td3.py:72-79)

#                 seed O   A   B     policy hidden  critic hidden  E  Oc
CASES = {
    "critic_only": (511, 5, 2, 67, [64, 64], [64, 64], 2, None),
    "full": (511, 5, 2, 67, [64, 64], [64, 64], 2, None),
    "ddpg": (512, 5, 2, 67, [64, 64], [64, 64], 1, None),
    "two_calls": (511, 5, 2, 67, [64, 64], [64, 64], 2, None),
    "critic_states": (513, 12, 3, 70, [64, 64], [64, 64], 2, 9),
    "narrow": (514, 5, 1, 1, [64], [64], 2, None),
    "act64": (515, 70, 64, 37, [128, 64, 64], [128, 64, 64], 2, 29),
    "split_ragged": (516, 45, 17, 4099, [256, 128], [256, 128], 2, None),
}
COMPOUNDING = ("two_calls", "split_ragged")         # held to max(bar, 2 x F32_GAP) (tests/test_gpu_td3.py)


class Case:
    def __init__(self, name):
        seed, O, A, B, ph, qh, E, Oc = CASES[name]
        self.name, self.seed, self.O, self.A, self.B, self.ph, self.qh, self.E, self.Oc = name, seed, O, A, B, ph, qh, E, O if Oc is None else Oc
        self.joint = name == "ddpg"
        p = tw.problem(seed, O, A, B, ph, qh, E, Oc)
        self.ps, self.qs, self.state, self.batch, self.cbatch, self.h = p["ps"], p["qs"], p["state"], p["batch"], p["cbatch"], p["h"]
        if self.joint:
            self.h = dict(self.h, smoothing_epsilon=0.0)
        self.eps = None if self.joint else np.random.default_rng(seed + 1).standard_normal((B, A)).astype(np.float32)
        # the calls the case makes, in order: (policy_step, lr_policy, lr_critic)
        self.calls = {"critic_only": [(False, LR, LR)], "two_calls": [(False, LR, LR), (True,) + LR2]}.get(name, [(True, LR, LR)])

    def descs(self):
        from rlx_amd.hip import mlp_desc
        return (mlp_desc(self.O, self.ph, self.A, nets.ACT_RELU, False, False), mlp_desc(self.Oc + self.A, self.qh, 1, nets.ACT_RELU, False, False))

    def _call(self, st, call, eps=None, **faults):
        pstep, lrp, lrq = call
        cb = self.cbatch or (None, None)
        if self.joint:
            return tw.ddpg_step(self.ps, self.qs, st, self.batch, self.h, lrp, lrq, TAU, cb[0], cb[1])
        return tw.update(self.ps, self.qs, st, self.batch, self.eps if eps is None else eps, self.h, lrp, lrq, TAU, pstep, cb[0], cb[1], **faults)

    def twin_call(self, st, call, eps=None, dtype=np.float64, **faults):
        """one call of the twin from st (its float32 values, evaluated in dtype) -> (new state, metrics, aux)"""
        return self._call(tw.cast_state(st, dtype), call, eps, **faults)

    def twin(self, dtype=np.float64, **faults):
        """all the case's calls in a row, each from the state the last one left (NOT rounded in between: compounding is the point)
        -> [(new state, metrics, aux) per call]"""
        out, st = [], tw.cast_state(self.state, dtype)
        for call in self.calls:
            out.append(self._call(st, call, **faults))
            st = out[-1][0]
        return out


def _rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30))


def metrics_vector(met):
    """a twin's metrics in rlx_td3_update_f32's order (NaN where the call has none)"""
    return [float(met.get(n, np.nan)) for n in tw.METRICS]


def figures(out, metrics, new, met, old):
    """a run (out: STATE_KEYS -> arrays, metrics [5]) -- or the float32 twin -- against the float64 twin's (new, met); old: the state
    the call(s) started from.  Without a policy step the policy's figures are absent (it must be unchanged, bit for bit)."""
    pstep = "loss/policy_loss" in met
    exp = metrics_vector(met)
    m = np.asarray(metrics, np.float64)
    f = {"metrics": max(abs(m[i] - exp[i]) / max(abs(exp[i]), 1.0) for i in ((0, 2, 3) if pstep else (0,))),
         "norms": max(abs(m[i] - exp[i]) / abs(exp[i]) for i in ((1, 4) if pstep else (1,)))}
    for k in ("pm", "qm", "pv", "qv") if pstep else ("qm", "qv"):
        f[k] = _rel(out[k], new[k])
    for k in ("P", "Q") if pstep else ("Q",):
        d = np.abs(np.asarray(out[k], np.float64) - new[k])
        f[k + "99"], f[k + "max"] = float(np.quantile(d, 0.99)), float(d.max())
    if pstep:
        for k in ("QT", "PT"):
            f[k] = float((np.abs(np.asarray(out[k], np.float64) - new[k]) - 1e-4 * np.abs(new[k])).max())
    return f


def f32_gap(c):
    """the twin in numpy float32 against the twin in float64 over all the case's calls (figures of the last call)"""
    new, met, _ = c.twin()[-1]
    new32, met32, _ = c.twin(np.float32)[-1]
    return figures(new32, metrics_vector(met32), new, met, c.state)


FAULTS = {"inner_clip_dropped": dict(inner_clip=False), "min_is_critic_0": dict(use_min=False),
          "targets_move_without_policy_step": dict(move_targets_always=True)}


def min_q_gap(c):
    """the smallest |Q1 - Q2| of the float64 twin on the policy step's rows (E = 2 and a policy step; else None)"""
    if c.E != 2:
        return None
    gaps = [float(np.abs(aux["qa"][:, 0] - aux["qa"][:, 1]).min()) for _, _, aux in c.twin() if "qa" in aux]
    return min(gaps) if gaps else None
