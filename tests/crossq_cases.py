"""Helpers shared by the shape tests of CrossQ (test_crossq_cases.py, test_gpu_crossq_shapes.py): one case table for
rlx_crossq_critic_update_f32 / rlx_crossq_policy_update_f32 across what cq_check_net, cq_check_hp and ens_prologue accept.

A case is test_gpu_crossq.py's Case -- crossq_twin.problem's recipe, its Run, figures, check and BARS -- from a row of the table
below instead of a row of its CASES.  nc = num_cus sizes many_rows alone.

| case        | O / Oc  | A  | policy hidden  | critic hidden  | E  | B           | dense_bias | what it is there for                               |
|-------------|---------|----|----------------|----------------|----|-------------|------------|----------------------------------------------------|
| act64       | 70 / 29 | 64 | (128, 64, 64)  | (128, 64, 64)  | 3  | 37          | 0          | A 64, Oc unaligned, Oc + A ragged, odd B           |
| wide_policy | 48 / 48 | 16 | (2048, 1984)   | (1984, 2048)   | 1  | 24          | 0.5        | widths at the limit, cq_dw's bands, a ragged band  |
| half_split  | 45 / 45 | 17 | (256, 128)     | (256, 128)     | 2  | 2049        | 0          | 2 B >= 4096 > B: only the joint pass goes split    |
| e16_cut     | 8 / 9   | 3  | (64, 128, 192) | (64, 128, 192) | 16 | 4099        | 3 (*)      | E 16, the image list ends inside critic 5          |
| many_rows   | 64 / 64 | 1  | (64)           | (64)           | 1  | 128 nc + 37 | 0          | slabs of 65 rows, BrnWalk::next, A 1               |
| ties        | 5 / 5   | 2  | (64, 64)       | (64, 64)       | 3  | 67          | 0          | critic 2 = critic 0: k_crossq_policy_seed's ties   |

(*) E16_DENSE_BIAS below has the measurements: with 0 every seed has units within float32 rounding of their ReLU kink.
Every case: brn_warmup_steps 100000 (not warmed), fresh running statistics.  Oc != O: critic_states / critic_next_states are passed.
A dense_bias case runs Adam with eps 1e-5 (test_gpu_crossq.py's docstring has the reason).  What each case is there for is
recomputed from tests/net_paths.py in test_crossq_cases.py.

SEEDS holds each case's seed: the first whose pair of updates is usable() (test_gpu_crossq.py's conditions) AND whose float32 twin
with double column sums is within half of every one-step bar of the float64 twin, so that max(bar, 2 gap) is the one-step bar (this
file run as a script scans them).  A seed that fails the second condition has a unit within float32 rounding of its ReLU kink.
The third condition: each of the three perturbed twins below misses a bar by more than ten times (faults_seen), so that the inputs
are ones on which the bars see a wrong tail.  ties asks a fourth: the copied pair holds the minimum in at least a quarter of the rows.

The perturbed twins (perturbed) are the faults the bars have to see: a tail row, a last column, a last network."""
import contextlib

import numpy as np

import crossq_twin as tw
import test_gpu_crossq as m

NAMES = ("act64", "wide_policy", "half_split", "e16_cut", "many_rows", "ties")
BARS = m.BARS
# case -> seed (0 where not listed): python tests/crossq_cases.py.  ties: seed 0 has the copied pair at the minimum in 12 of 67 rows
# (critic 1 lies lower), under the quarter the case asks for; seed 1 in 33.  e16_cut: seed 0 is usable() and fails the second condition
# (metrics 1.4, qm 1.8 bars); seed 1 is within 0.05 bars everywhere.  many_rows: on seed 0 the last of the joint pass's 65610 rows is a
# mild one -- left out of the column sums it moves qm by 4.8 bars, under the third condition's ten; on seed 1 by 17 (of the seeds
# 0 .. 23 only 0 and 16 stay under ten; the others read 11 to 44)
SEEDS = {"e16_cut": 1, "many_rows": 1, "ties": 1}
# e16_cut's dense_bias.  With 0, 16 critics x 8198 rows x 384 units put 50 M pre-activations of the joint pass around their ReLU kink:
# on each of the seeds 7 .. 15 about 40 of them lie within 1e-6 of it (a dozen within 3e-7), and ONE derivative taken on the other side
# moves the critics' first moments by up to 20 bars.  Measured: the double-sum float32 twin is 0.9 to 12.9 bars off in qm on seeds 0 .. 6;
# on seed 7 it is within 0.11 bars, and the device -- same seed, another rounding -- read qm 8.6e-5 on the split-operand engine and
# 9.2e-5 on the exact one, every critic within 3e-6 of the twin but critics 12 and 15 (and 1, 3, 5 on the exact engine), their whole
# difference in ONE unit's column of the third Dense's gradient: critic 12's unit 86 has z = -7.6e-8 in row 3416, critic 15's unit 52
# z = +7.3e-8 in row 5597, the smallest |z| of their layers, and the float64 twin with that one derivative flipped is 2.0e-7 / 1.9e-7
# from the device.  No seed is free of such units, so the case cannot be seeded into shape; a Dense bias of 3 moves the pre-activations
# to 3 +- 1 and leaves none within 1e-6 of the kink (min_preactivation; asserted in test_crossq_cases.py).  What the case is there for
# -- E 16, both image lists ending inside critic 5, the minimum over 16 critics -- does not depend on it.
E16_DENSE_BIAS = 3.0
SCAN = 20          # a case that meets the two conditions on none of its first SCAN usable seeds is changed in size


def table_row(name, num_cus=256):
    """-> a row in test_gpu_crossq.CASES' form: O, A, B, policy hidden, critic hidden, E, Oc, warm-up, stats_away, dense_bias"""
    return {
        "act64": (70, 64, 37, [128, 64, 64], [128, 64, 64], 3, 29, 100000, False, 0.0),
        "wide_policy": (48, 16, 24, [2048, 1984], [1984, 2048], 1, None, 100000, False, 0.5),
        "half_split": (45, 17, 2049, [256, 128], [256, 128], 2, None, 100000, False, 0.0),
        "e16_cut": (8, 3, 4099, [64, 128, 192], [64, 128, 192], 16, 9, 100000, False, E16_DENSE_BIAS),
        "many_rows": (64, 1, 128 * num_cus + 37, [64], [64], 1, None, 100000, False, 0.0),
        "ties": (5, 2, 67, [64, 64], [64, 64], 3, None, 100000, False, 0.0),
    }[name]


def shape_case(name, num_cus=256, seed=None):
    row = table_row(name, num_cus)
    c = m.Case(name, SEEDS.get(name, 0) if seed is None else seed, row)
    c.ph, c.qh, c.asym = list(row[3]), list(row[4]), row[6] is not None
    if name == "ties":                                 # critic 2 is critic 0, parameters and statistics
        n, s = c.qs.n_params, c.qs.n_stats
        c.state = dict(c.state, qp=c.state["qp"].copy(), qs=c.state["qs"].copy())
        c.state["qp"][2 * n:3 * n], c.state["qs"][2 * s:3 * s] = c.state["qp"][:n], c.state["qs"][:s]
    return c


def tied_rows(c, mid):
    """rows of the policy update (from the state `mid` the critic update left) in which more than one critic holds the minimum"""
    cfg = tw.cfg_of(c.h)
    head, _, _ = tw.net_forward(c.ps, mid["pp"], mid["ps"], c.batch[0].astype(np.float64), True, False, cfg)
    a = tw.sample(head, c.eps[1].astype(np.float64), c.h["log_std_min"], c.h["log_std_max"])[0]
    x = np.concatenate([(c.batch if c.cbatch is None else c.cbatch)[0].astype(np.float64), a], axis=1)
    n, s = c.qs.n_params, c.qs.n_stats
    qa = np.stack([tw.net_forward(c.qs, mid["qp"][e * n:(e + 1) * n], mid["qs"][e * s:(e + 1) * s], x, False, False, cfg)[0][:, 0] for e in range(c.E)], axis=1)
    return (qa == qa.min(axis=1, keepdims=True)).sum(axis=1) > 1


def min_preactivation(c, a2=None):
    """the smallest |z| over the hidden pre-activations of the critics' joint training pass (float64 twin): how far the nearest unit is
    from the kink at which float32 rounding decides its derivative"""
    cfg = tw.cfg_of(c.h)
    f8 = lambda v: np.asarray(v, np.float64)
    a2 = tw.critic_update(c.ps, c.qs, c.state, c.batch, c.cbatch, c.eps[0], c.h)[2]["a2"] if a2 is None else a2     # a' ~ pi(s')
    cs, cs2 = (f8(v) for v in (c.cbatch or c.batch[:2]))
    x = np.concatenate([np.concatenate([cs, f8(c.batch[2])], axis=1), np.concatenate([cs2, a2], axis=1)], axis=0)
    n, s, least = c.qs.n_params, c.qs.n_stats, np.inf
    for e in range(c.E):
        p = c.state["qp"][e * n:(e + 1) * n]
        caches = tw.net_forward(c.qs, p, c.state["qs"][e * s:(e + 1) * s], x, True, False, cfg)[1]
        for l in range(c.qs.L):
            z = caches[l]["y"] @ caches[l]["W"] + p[c.qs.b[l]:c.qs.b[l] + c.qs.dims[l + 1]]
            least = min(least, float(np.abs(z).min()))
    return least


# ------------------------------------------------------------------------------------------------- the faults the bars must see
@contextlib.contextmanager
def _patched(name, wrap):
    old = getattr(tw, name)
    setattr(tw, name, wrap(old))
    try:
        yield
    finally:
        setattr(tw, name, old)


def perturbed(c, what):
    """a context in which the twin is wrong in one of three ways a kernel can be:
       "tail_row"    the last row of the critics' joint pass of 2 B rows is left out of the BRN column sums (sum x, sum x^2 over 2 B - 1
                     rows, divided by 2 B): a short last slab of k_brn_colsum dropped
       "last_column" the last action column of dQ/da is zero in the policy update
       "last_net"    the last critic is evaluated, forward and backward, in both updates, on the parameters of the one before it"""
    if what == "tail_row":
        def wrap(stats):
            def f(x):
                if x.shape[0] != 2 * c.B:
                    return stats(x)
                mu = x[:-1].sum(axis=0) / x.shape[0]
                return mu, np.maximum(0, (x[:-1] * x[:-1]).sum(axis=0) / x.shape[0] - mu * mu)
            return f

        def wrap_bwd(backward):
            def f(dY, cache, relu_mask=False, **k):
                if dY.shape[0] != 2 * c.B:
                    return backward(dY, cache, relu_mask, **k)
                short = dY.copy()
                short[-1] = 0                                  # sum dY and sum dY x without the row; its own dY g rho stays
                dX, dg, db = backward(short, cache, relu_mask, **k)
                dX[-1] += dY[-1] * cache["g"] * cache["rho"] * ((cache["x"][-1] > 0) if relu_mask else 1)
                return dX, dg, db
            return f
        stack = contextlib.ExitStack()
        stack.enter_context(_patched("brn_batch_stats", wrap))
        stack.enter_context(_patched("brn_backward", wrap_bwd))
        return stack
    if what == "last_column":
        def wrap(backward):
            def f(spec, *a, **k):
                g, dx = backward(spec, *a, **k)
                if spec is c.qs:
                    dx = dx.copy()
                    dx[:, -1] = 0
                return g, dx
            return f
        return _patched("net_backward", wrap)
    assert what == "last_net" and c.E > 1

    def wrap(update):
        def f(ps, qs, st, *a, **k):
            qp = st["qp"].copy()
            qp[-qs.n_params:] = qp[-2 * qs.n_params:-qs.n_params]
            return update(ps, qs, dict(st, qp=qp), *a, **k)
        return f
    stack = contextlib.ExitStack()
    stack.enter_context(_patched("critic_update", wrap))
    stack.enter_context(_patched("policy_update", wrap))
    return stack


PERTURBATIONS = ("tail_row", "last_column", "last_net")


# the figure each fault lands in: a dropped row of the column sums moves the advanced statistics, or the critics' gradient
LANDS_IN = {"tail_row": ("qs", "qm"), "last_column": ("pm",), "last_net": ("qm",)}


def fault_ratios(c, what, new, met):
    """figure / bar of the float64 twin under perturbed(c, what) against the right twin's (new, met) -> {figure: ratio}"""
    with perturbed(c, what):
        _, bad, bad_met, _ = c.twin(c.state)
    return {k: v / BARS[k] for k, v in m.figures(bad, m.metrics_vector(bad_met), new, met).items()}


def faults_seen(c, new, met):
    """the third condition of SEEDS: every fault misses the bar of a figure it lands in by more than ten times"""
    return all(max(fault_ratios(c, w, new, met)[k] for k in LANDS_IN[w]) > 10 for w in PERTURBATIONS if w != "last_net" or c.E > 1)


def gap_ok(c, ref=None):
    """the second condition of SEEDS -> (holds, the figures)"""
    gap = m.f32_gap(c, ref=ref)
    return all(v <= 0.5 * BARS[k] for k, v in gap.items()), gap


if __name__ == "__main__":      # SEEDS (CPU only)
    found = {}
    for name in NAMES:
        tried = 0
        for seed in range(200):
            c = shape_case(name, seed=seed)
            if not c.usable():
                continue
            tried += 1
            ok, gap = gap_ok(c)
            ok = ok and faults_seen(c, *c.twin(c.state)[1:3])
            if name == "ties":
                tied = int(tied_rows(c, c.twin(c.state)[0]).sum())
                print(f"ties seed {seed}: {tied} tied rows of {c.B}")
                ok = ok and 4 * tied >= c.B
            print(f"{name} seed {seed}: " + " ".join(f"{k} {v / BARS[k]:.2f}" for k, v in gap.items() if v > 0.1 * BARS[k]) + (" ok" if ok else " -"), flush=True)
            if ok or tried == SCAN:
                break
        assert ok, name
        found[name] = seed
    print("SEEDS =", {n: s for n, s in found.items() if s})
