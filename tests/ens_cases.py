"""Helpers shared by the shape tests of the ensemble-SAC family (test_ens_cases.py, test_gpu_ens_shapes.py): one case table for
rlx_redq_update_f32, rlx_aqe_update_f32, rlx_droq_update_f32 and rlx_tqc_update_f32 across what ens_check_net / ens_prologue accept.

A case is built on the Case / Run / figures / check of the algorithm's own file (test_gpu_redq.py, test_gpu_aqe.py, test_gpu_droq.py,
test_gpu_tqc.py) -- their input recipes (redq_twin.problem and its siblings), learning rates, BARS and the rule max(bar, 2 F32_GAP) --
from a row of the table below instead of a row of their CASES.  nc = num_cus sizes many_rows alone.

| case         | seed | O / Oc  | A            | policy hidden  | critic hidden (DroQ)           | E, M                    | G | B          | AQE H, dropped | TQC N, dropped per net |
|--------------|------|---------|--------------|----------------|--------------------------------|-------------------------|---|------------|----------------|------------------------|
| narrow       | 411  | 5 / 5   | 1            | (64)           | (64)                           | 2, 1                    | 2 | 1          | 1, 1           | 2, 1                   |
| wide         | 412  | 48 / 48 | 16 (DroQ 27) | (1024, 128)    | (1024, 768) ((768, 704))       | 2, 2                    | 1 | 37         | 8, 3           | 25, 2                  |
| act64        | 413  | 70 / 29 | 64           | (128, 64, 64)  | (128, 64, 64) ((128, 320, 64)) | 3, 2 (AQE E 16; TQC E 4) | 2 | 37         | 8, 100         | 32, 3                  |
| split_ragged | 414* | 45 / 45 | 17           | (256, 128)     | (256, 128)                     | 2, 2                    | 2 | 4099       | 3, 2           | 25, 2                  |
| cut_inside   | 415  | 8 / 9   | 3            | (64, 128, 192) | (64, 128, 192)                 | 6, 2                    | 1 | 4099       | 2, 3           | 5, 1                   |
| many_rows    | 416  | 64 / 64 | 40           | (64)           | (64)                           | 2, 2                    | 1 | 64 nc + 37 | 40, 5          | 40, 3                  |

Oc != O: critic_states / critic_next_states are passed.  TQC has no M and no G.  DroQ's rate is 0.25.  The inputs are drawn from the
seed, the injected noise from seed + 1 (* DroQ's split_ragged: 424, see SEEDS).  What each case is there for is recomputed from tests/net_paths.py in test_ens_cases.py.

The perturbed twins (perturbed) are the faults the bars have to see: a tail row, a last column, a last network."""
import contextlib

import numpy as np

import aqe_twin
import droq_twin
import redq_twin
import test_gpu_aqe as m_aqe
import test_gpu_droq as m_droq
import test_gpu_redq as m_redq
import test_gpu_tqc as m_tqc
import tqc_twin
from oracle import nets, prng

ALGOS = ("redq", "aqe", "droq", "tqc")
NAMES = ("narrow", "wide", "act64", "split_ragged", "cut_inside", "many_rows")
MODS = {"redq": m_redq, "aqe": m_aqe, "droq": m_droq, "tqc": m_tqc}
KEY = m_redq.KEY
RATE = 0.25
BARS = m_redq.BARS          # (test_gpu_aqe.py's are the same numbers, test_gpu_droq.py imports these; test_gpu_tqc.py: check_first_step)
SEEDS = {"narrow": 411, "wide": 412, "act64": 413, "split_ragged": 414, "cut_inside": 415, "many_rows": 416,
         # DroQ's split_ragged from 414: the float32 twin is 1.3e-5 off in the policy's first moments, past their 1e-5 (over 4099 rows one
         # unit sits within float32 rounding of its kink); from 424 it is 2.6e-7 off
         ("droq", "split_ragged"): 424}

# figures() of the twin in numpy float32 against the twin in float64 on each case's inputs (test_ens_cases.py measures them and holds
# each to half of its bar; this file run as a script prints them).  A figure missing here is below a tenth of its one-step bar.  The
# second moments' 1.3e-5 is float32's 1 - 0.999 against 0.001, the same in every float32 Adam (test_gpu_redq.py); twice it is below
# their 5e-5: every case meets the one-step bars unchanged.
PV_QV = {"pv": 1.3e-05, "qv": 1.3e-05}
F32_GAP = {a: {n: dict(PV_QV) for n in NAMES} for a in ALGOS}


def table_row(name, num_cus=256):
    """-> dict of the table's columns for one case"""
    O, Oc, A, A_droq, ph, qh, qh_droq, E, E_aqe, E_tqc, M, G, B, H, Hdrop, N, Ndrop = {
        "narrow": (5, None, 1, 1, (64,), (64,), (64,), 2, 2, 2, 1, 2, 1, 1, 1, 2, 1),
        "wide": (48, None, 16, 27, (1024, 128), (1024, 768), (768, 704), 2, 2, 2, 2, 1, 37, 8, 3, 25, 2),
        "act64": (70, 29, 64, 64, (128, 64, 64), (128, 64, 64), (128, 320, 64), 3, 16, 4, 2, 2, 37, 8, 100, 32, 3),
        "split_ragged": (45, None, 17, 17, (256, 128), (256, 128), (256, 128), 2, 2, 2, 2, 2, 4099, 3, 2, 25, 2),
        "cut_inside": (8, 9, 3, 3, (64, 128, 192), (64, 128, 192), (64, 128, 192), 6, 6, 6, 2, 1, 4099, 2, 3, 5, 1),
        "many_rows": (64, None, 40, 40, (64,), (64,), (64,), 2, 2, 2, 2, 1, 64 * num_cus + 37, 40, 5, 40, 3),
    }[name]
    return dict(O=O, Oc=Oc, A=A, A_droq=A_droq, ph=ph, qh=qh, qh_droq=qh_droq, E=E, E_aqe=E_aqe, E_tqc=E_tqc, M=M, G=G, B=B, H=H,
                Hdrop=Hdrop, N=N, Ndrop=Ndrop)


class EnsCase:
    """one case of one algorithm: the algorithm's own Case (self.c) and what differs between the four files behind one interface"""

    def __init__(self, algo, name, num_cus=256):
        t = table_row(name, num_cus)
        self.algo, self.name, self.mod, seed = algo, name, MODS[algo], SEEDS.get((algo, name), SEEDS[name])
        ph, qh = list(t["ph"]), list(t["qh_droq"] if algo == "droq" else t["qh"])
        if algo == "redq":
            self.c = m_redq.Case((t["O"], t["A"], t["B"], ph, qh, t["E"], t["M"], t["G"], t["Oc"], 0.0), name, seed)
        elif algo == "aqe":
            self.c = m_aqe.Case((t["O"], t["A"], t["B"], ph, qh, t["E_aqe"], t["H"], t["Hdrop"], t["G"], t["Oc"], 0.0), name, seed)
        elif algo == "droq":
            self.c = m_droq.Case((t["O"], t["A_droq"], t["B"], ph, qh, t["E"], t["M"], t["G"], t["Oc"], 0.0, RATE), name, seed)
        else:
            self.c = m_tqc.Case(t["O"], t["A"], t["B"], ph, qh, t["E_tqc"], t["N"], t["Ndrop"], t["Oc"], seed=seed)
            rng = np.random.default_rng(seed + 1)
            self.c.eps = (rng.standard_normal((self.c.B, self.c.A)).astype(np.float32), rng.standard_normal((self.c.B, self.c.A)).astype(np.float32))
            self.c.name = name
        self.c.gap = F32_GAP[algo][name]
        c = self.c
        self.ph, self.qh = ph, qh
        self.O, self.Oc, self.A, self.B, self.E = c.O, c.Oc, c.A, c.B, c.E
        self.G = 1 if algo == "tqc" else c.G
        self.M = {"redq": t["M"], "droq": t["M"], "aqe": c.E, "tqc": c.E}[algo]
        self.heads = {"redq": 1, "droq": 1, "aqe": t["H"], "tqc": t["N"]}[algo]        # a critic's outputs
        self.asym = c.cbatch is not None

    def bars(self):
        return {k: max(b, 2 * self.c.gap.get(k, 0.0)) for k, b in BARS.items()}

    def extras(self, key=KEY, scheme=1):
        """the inputs of the twin besides state and noise, from the oracle's key chain: REDQ's subsets, DroQ's subsets and masks"""
        if self.algo == "redq":
            return (self.c.subsets(key, scheme),)
        if self.algo == "droq":
            return (self.c.subsets(key, scheme), self.c.masks(key, scheme))
        return ()

    def twin(self, extras=None, dtype=np.float64):
        """the algorithm's twin from the case's state on its noise -> (new state, metrics, ...)"""
        extras = self.extras() if extras is None else extras
        return self.c.twin(self.c.state, self.c.eps, *extras, dtype)

    def figures(self, out, metrics, new, met):
        return m_redq.figures(out, metrics, new, met)

    def f32_gap(self):
        """the twin in numpy float32 against the twin in float64, same inputs (figures())"""
        ex = self.extras()
        new, met = self.twin(ex)[:2]
        new32, met32 = self.twin(ex, np.float32)[:2]
        return self.figures(new32, m_redq.twin_metrics_vector(met32), new, met)

    def run(self, ctx, dev, inject=True, prof=False, key=KEY):
        return self.mod.Run(ctx, dev, self.c, self.c.state, key, 1, inject=self.c.eps if inject else None, prof=prof)

    def tqc_key(self, key=KEY, scheme=1):
        """rlx_tqc_update_f32's returned key: split(key, 2 B + 1)[0] (tqc.py:211)"""
        return prng.split(np.asarray(key, np.uint32), 2 * self.B + 1, bool(scheme))[0]


def shape_case(algo, name, num_cus=256):
    return EnsCase(algo, name, num_cus)


# ------------------------------------------------------------------------------------------------- the faults the bars must see
def _patched(pairs):
    @contextlib.contextmanager
    def cm():
        old = [(o, n, getattr(o, n)) for o, n, _ in pairs]
        try:
            for o, n, f in pairs:
                setattr(o, n, f(getattr(o, n)))
            yield
        finally:
            for o, n, f in old:
                setattr(o, n, f)
    return cm()


def _without_tail_row(loss_fn, dq_index):
    def f(*a, batch=None, **k):
        out = list(loss_fn(*a, **k) if batch is None else loss_fn(*a, batch=batch, **k))
        if batch is None:                              # (tqc_twin.pair_loss calls itself on parts of a large batch)
            dq = out[dq_index].copy()
            dq[-1] = 0
            out[dq_index] = dq
        return tuple(out)
    return f


def _without_last_column(backward):
    def f(*a, **k):
        out = backward(*a, **k)
        if not k.get("need_dx"):
            return out
        dx = out[1].copy()
        dx[:, -1] = 0
        return out[0], dx
    return f


def _last_net_from_the_one_before(step, qs_at, qp_at):
    def f(*a, **k):
        a = list(a)
        n, qp = a[qs_at].n_params, a[qp_at].copy()
        qp[-n:] = qp[-2 * n:-n]
        a[qp_at] = qp
        return step(*a, **k)
    return f


def perturbed(algo, what):
    """a context in which the algorithm's twin is wrong in one of three ways a kernel can be:
       "tail_row"    the last row of the batch is left out of every critic step's gradient (its d loss / d q is zero)
       "last_column" the last action column of dQ/da is zero in the policy step
       "last_net"    the last online critic is evaluated, forward and backward, with the parameters of the one before it"""
    if what == "tail_row":
        return _patched({"redq": [(redq_twin, "critic_loss", lambda g: _without_tail_row(g, 2))],
                         "droq": [(redq_twin, "critic_loss", lambda g: _without_tail_row(g, 2))],
                         "aqe": [(aqe_twin, "critic_loss", lambda g: _without_tail_row(g, 2))],
                         "tqc": [(tqc_twin, "pair_loss", lambda g: _without_tail_row(g, 1))]}[algo])
    if what == "last_column":
        return _patched([(droq_twin, "critic_backward", _without_last_column)] if algo == "droq" else [(nets, "backward", _without_last_column)])
    assert what == "last_net"
    if algo == "tqc":
        return _patched([(tqc_twin, "loss_and_grads", lambda g: _last_net_from_the_one_before(g, 2, 3))])
    tw = {"redq": redq_twin, "aqe": aqe_twin, "droq": droq_twin}[algo]
    return _patched([(tw, "critic_step", lambda g: _last_net_from_the_one_before(g, 1, 3)),
                     (tw, "policy_step", lambda g: _last_net_from_the_one_before(g, 1, 3))])


PERTURBATIONS = ("tail_row", "last_column", "last_net")

if __name__ == "__main__":      # the float32 gaps behind F32_GAP (CPU only)
    for algo in ALGOS:
        for name in NAMES:
            gap = shape_case(algo, name).f32_gap()
            print(f"{algo:5s} {name:13s}", " ".join(f"{k} {v:.1e}" for k, v in gap.items()))
