"""Helpers shared by the FastTD3 tests (test_gpu_fasttd3.py, test_fasttd3_cases.py, test_gpu_fasttd3_shapes.py): the ReLU-kink /
tie accounting of the 1e-5 gradient bar, the library's hyperparameter struct from a dict, a Case (a float64 twin state of
float32-representable values, a batch with terminations, truncations and n-steps 1..4, noise per step), a Run (one
rlx_fasttd3_critic_update_f32 and one rlx_fasttd3_policy_update_f32 call on device copies of a state) and the comparison.

Both updates of a Run start from the SAME state (the policy update sees the critics from before the critic update): the twin
and the device get bit-identical float32 inputs in both, and each bar measures one update's kernels.

Bars (the ones test_gpu_fasttd3.py holds the kernels to): gradients 1e-5 relative in L2 per vector -- defined where the fp32
gradient is, see KINK_TAU below -- and 2e-5 per parameter block; first moments 1e-5; second moments 2e-5 (v is quadratic in g:
twice the gradient bar), both on what the step added to the given m0 / v0; parameters and targets after the step 1e-5; scalars
1e-5 relative, with a floor max(1, max|v| / 10) only for q_min / q_max and the policy loss (means of expected values that large)."""
import numpy as np
import torch

import fasttd3_twin as tw
from oracle.fastsac import adamw, clip_grad_norm, polyak
from rlx_amd.hip import FastTd3Hparams, relu_mlp_desc
from shape_batch import draw_batch, index_sets
from shape_batch import f32 as _f32


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _hp(h, nr_atoms, clipped):
    hp = FastTd3Hparams()
    for k in ("gamma", "tau", "v_min", "v_max", "weight_decay", "smoothing_epsilon", "smoothing_clip_value", "max_grad_norm"):
        setattr(hp, k, float(h[k]))
    hp.lr_policy = hp.lr_critic = float(h["learning_rate"])
    hp.adam_b1, hp.adam_b2, hp.adam_eps = 0.9, 0.999, 1e-8
    hp.nr_atoms, hp.clipped_double_q = int(nr_atoms), int(bool(clipped))
    return hp


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _kinks(flat, in_dim, hidden, x, tau=8e-6):
    """[(|z| / rms, row, layer, unit)] of the ReLU pre-activations of the batch within tau of zero relative to their row's RMS
    (float64): a unit-sample within fp32 rounding of its kink has an undefined fp32 gradient -- any fp32 evaluation may land on
    either side, and that sample's whole backward contribution through the unit flips with it."""
    h, off, d, out = x.astype(np.float64), 0, in_dim, []
    for li, w in enumerate(hidden):
        W = flat[off:off + d * w].reshape(d, w); off += d * w
        z = h @ W + flat[off:off + w]; off += w
        m = np.abs(z) / np.sqrt((z * z).mean(axis=1, keepdims=True))
        out += [(float(m[i, j]), int(i), li, int(j)) for i, j in zip(*np.nonzero(m < tau))]
        h, d = np.maximum(z, 0.0), w
    return out


def _fwd_flip(flat, in_dim, hidden, out_dim, x, flips):
    """the twin's ReLU network on ONE row with the on / off state of the units `flips` ({(layer, unit)}) inverted"""
    off, d, h = 0, in_dim, x
    for li, w in enumerate(list(hidden) + [out_dim]):
        W = flat[off:off + d * w].reshape(d, w); off += d * w
        z = h @ W + flat[off:off + w]; off += w
        if li < len(hidden):
            m = (z > 0).to(z.dtype)
            for (l, j) in flips:
                if l == li:
                    m[0, j] = 1.0 - m[0, j]
            z = z * m
        h, d = z, w
    return h


def _explain(gd, ge, cands, delta, limit):
    """Which kink / tie candidates did the device evaluate on their other side?  Candidates are taken closest to their kink first;
    one is taken when its alternative -- ge + delta(cand): the twin's gradient with that one unit-sample / row choice inverted --
    brings the device result closer (by more than 0.1 %).  That is the test 2 r.d > |d|^2 for the residual r = gd - ga: a
    candidate that did not flip on the device has no component in r, so it is not taken; flips are independent samples, so their
    alternatives add.  -> (adjusted expectation, taken candidates)"""
    ga, taken = ge.copy(), []
    for c in sorted(cands, key=lambda c: c[0]):
        if _rel(gd, ga) < 1e-6 or len(taken) >= limit:
            break
        alt = ga + delta(c)
        if _rel(gd, alt) < 0.999 * _rel(gd, ga):
            ga, taken = alt, taken + [c]
    return ga, taken


# ReLU kink window (|z| / row RMS of the float64 pre-activation) and the number of flips allowed per update step.  Measured on
# test_gpu_fasttd3.py's clipped policy step at the default batch: a plain float32 evaluation of the formula (torch on the CPU) is
# 3.5e-5 from float64, and 7.9e-8 once it takes its ReLU masks from float64 -- the whole difference is 10 unit-samples on the other
# side of their kink (1 in the policy, 9 in the critics), at margins 8e-9 .. 8.4e-7; the exact-fp32 and split-operand engines land
# at 3.5e-5 and 3.7e-5 on the same inputs before any flip is accounted for.  On the MI355X (split-operand engine) those steps take
# 3 .. 4 flips (critic steps; mean-of-two policy step) and 13 in the clipped policy step, 4.2e-5 -> 5.7e-6; the first of those 13 is the
# policy's unit-sample that the CPU float32 evaluation flips too.
KINK_TAU = 4e-6
MAX_FLIPS = 16

HP = dict(gamma=0.97, tau=0.1, v_min=-10.0, v_max=10.0, learning_rate=3e-4, weight_decay=0.1, smoothing_epsilon=0.2,
          smoothing_clip_value=0.5, max_grad_norm=-1.0)
CRITIC_KEYS = ("Q", "qm", "qv", "QT")
POLICY_KEYS = ("P", "pm", "pv")
STATE_KEYS = POLICY_KEYS + CRITIC_KEYS
B1, B2 = 0.9, 0.999


def _T(x):
    return torch.tensor(np.asarray(x, dtype=np.float64))


class Case:
    """seeded per case.  O: the observation width, Op / Oc: the columns the policy / the critics see (index sets drawn from the
    seed; None: all of them -- then no critic_states are passed)"""

    def __init__(self, seed, O, A, policy_hidden, critic_hidden, NA, B, Op=None, Oc=None, clipped=True, **hp):
        self.h = dict(HP, **hp)
        rng = np.random.default_rng(seed)
        self.O, self.A, self.NA, self.B, self.clipped = O, A, NA, B, clipped
        self.ph, self.ch = tuple(policy_hidden), tuple(critic_hidden)
        self.pidx, self.cidx = index_sets(rng, O, Op, Oc)
        self.Op, self.Oc = (O if Op is None else Op), (O if Oc is None else Oc)
        self.split = self.pidx is not None or self.cidx is not None
        self.pd, self.qd = relu_mlp_desc(self.Op, self.ph, A), relu_mlp_desc(self.Oc + A, self.ch, NA)
        p, q = tw.make_params(seed, self.Op, A, NA, self.Oc, self.ph, self.ch)
        p, q = p.astype(np.float64), [x.astype(np.float64) for x in q]
        zp, zq = np.zeros(p.size), np.zeros(2 * q[0].size)
        self.state = dict(P=p, pm=zp, pv=zp, Q=np.concatenate(q[:2]), qm=zq, qv=zq, QT=np.concatenate(q[2:]))
        self.batch, self.cbatch = draw_batch(rng, B, O, A, self.h, lambda z: np.clip(0.6 * z, -1, 1), self.pidx, self.cidx)   # the policy's columns, the critics'
        self.rng = rng

    def noise(self):
        return _f32(self.rng.standard_normal((self.B, self.A)))

    def kw(self):
        return dict(policy_hidden=self.ph, critic_hidden=self.ch)

    def cstates(self):
        return self.batch[0] if self.cbatch is None else self.cbatch[0]

    def steps(self, st, eps, **kw):
        """the twin's (critic_step, policy_step) dicts from `st`; kw: their dtype= / trace= arguments"""
        nq = st["Q"].size // 2
        q = [st["Q"][:nq], st["Q"][nq:], st["QT"][:nq], st["QT"][nq:]]
        rc = tw.critic_step(st["P"], *q, self.Oc, self.A, self.NA, self.batch, eps, self.h, self.clipped, self.cbatch, **self.kw(), **kw)
        rp = tw.policy_step(st["P"], q[0], q[1], self.Oc, self.A, self.NA, self.batch[0], self.h, self.clipped,
                            None if self.cbatch is None else self.cbatch[0], **self.kw(), **kw)
        return rc, rp

    def apply(self, st, step, rc, rp, gq=None, gp=None):
        """clip_grad_norm_ + AdamW (+ Polyak) from the gradients gq / gp (default: the twin's) -> (new state, critic metrics [4],
        policy metrics [2])"""
        h = self.h
        gq = np.concatenate([rc["g_q1"], rc["g_q2"]]) if gq is None else gq
        gp = rp["g_policy"] if gp is None else gp
        gqc, qn = clip_grad_norm(gq, h["max_grad_norm"])
        gpc, pn = clip_grad_norm(gp, h["max_grad_norm"])
        qp, qm, qv = adamw(st["Q"], gqc, st["qm"], st["qv"], step, h["learning_rate"], h["weight_decay"], B1, B2)
        pp, pm, pv = adamw(st["P"], gpc, st["pm"], st["pv"], step, h["learning_rate"], h["weight_decay"], B1, B2)
        new = dict(P=pp, pm=pm, pv=pv, Q=qp, qm=qm, qv=qv, QT=polyak(st["QT"], qp, h["tau"]))
        return new, np.array([rc["q_loss"], rc["q_min"], rc["q_max"], qn]), np.array([rp["policy_loss"], pn])

    def run(self, ctx, dev, st, eps, step, key=(0, 7), profile=False):
        return Run(ctx, dev, self, st, eps, step, key, profile)


class Run:
    """rlx_fasttd3_critic_update_f32, then rlx_fasttd3_policy_update_f32 against the critics from BEFORE it, on device copies of a
    state.  prof: ctx.prof_rows() of each update (taken when `profile`)."""

    def __init__(self, ctx, dev, c, st, eps, step, key=(0, 7), profile=False):
        d = {k: _t(st[k], dev) for k in STATE_KEYS}
        q0 = d["Q"].clone()
        hp = _hp(c.h, c.NA, c.clipped)
        batch = tuple(_t(x, dev) for x in c.batch)
        cb = (None, None) if c.cbatch is None else tuple(_t(x, dev) for x in c.cbatch)
        self.cmet, self.pmet = torch.zeros(4, device=dev), torch.zeros(2, device=dev)
        self.eps = _t(eps, dev)                             # kept alive: the library holds the pointer
        self.prof = [None, None]
        ctx.dbg_set_sac_noise(self.eps, None)
        try:
            if profile:
                ctx.prof_begin()
            self.key, self.ccount = ctx.fasttd3_critic_update(c.pd, d["P"], c.qd, d["Q"], d["qm"], d["qv"], d["QT"], batch,
                                                              np.array(key, np.uint32), step - 1, hp, self.cmet, critic_states=cb[0],
                                                              critic_next_states=cb[1])
            if profile:
                ctx.prof_end()
                self.prof[0] = ctx.prof_rows()
                ctx.prof_begin()
            self.pcount = ctx.fasttd3_policy_update(c.pd, d["P"], d["pm"], d["pv"], c.qd, q0, batch[0], step - 1, hp, self.pmet,
                                                    critic_states=cb[0])
            if profile:
                ctx.prof_end()
                self.prof[1] = ctx.prof_rows()
        finally:
            ctx.dbg_set_sac_noise(None, None)
        torch.cuda.synchronize()
        self.out = {k: d[k].cpu().numpy().astype(np.float64) for k in STATE_KEYS}
        self.cmetrics, self.pmetrics = self.cmet.cpu().numpy().astype(np.float64), self.pmet.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------- kink / tie candidates of a Case
def clip_scale(g, max_norm):
    return 1.0 if max_norm == -1.0 else min(1.0, max_norm / (float(np.linalg.norm(g)) + 1e-6))


def critic_candidates(c, st, rc):
    """(candidates, delta) of the critic step from `st`: ReLU unit-samples of both online critics within KINK_TAU of their kink and,
    with clipped double Q, rows whose two projections' expectations tie -- counted from float64 alone; delta(cand) = the twin's
    gradient [q1 | q2] with that one unit-sample / row choice inverted, minus the twin's"""
    nq = st["Q"].size // 2
    q64 = [st["Q"][:nq], st["Q"][nq:]]
    Oc, A, NA, B = c.Oc, c.A, c.NA, c.B
    x = np.concatenate([c.cstates(), c.batch[2]], 1)
    tgt = [rc["target1"], rc["target2"]]

    def row_grad(k, row, flips, t_row):
        Qk = _T(q64[k]).requires_grad_(True)
        lg = _fwd_flip(Qk, Oc + A, c.ch, NA, _T(x[row:row + 1]), flips)
        (-(_T(t_row) * torch.log_softmax(lg, dim=1)).sum() / B).backward()
        return Qk.grad.numpy()
    cands = [(k_[0], "relu", k) + k_[1:] for k in range(2) for k_ in _kinks(q64[k], Oc + A, c.ch, x, KINK_TAU)]
    if c.clipped:
        tie = np.abs(rc["v1"] - rc["v2"]) / np.sqrt(0.5 * (rc["v1"] ** 2 + rc["v2"] ** 2).mean())
        # (a row whose two projections are the same distribution -- a terminal one: no next state in it -- has nothing to choose)
        cands += [(float(tie[i]), "tie", -1, int(i)) for i in np.nonzero(tie < KINK_TAU)[0] if np.abs(rc["p1"][i] - rc["p2"][i]).max() > 1e-12]

    def delta(cd):
        d = np.zeros(2 * nq)
        if cd[1] == "relu":
            _, _, k, row, li, j = cd
            d[k * nq:(k + 1) * nq] = row_grad(k, row, {(li, j)}, tgt[k][row:row + 1]) - row_grad(k, row, set(), tgt[k][row:row + 1])
        else:
            row = cd[3]
            other = rc["p2"][row:row + 1] if rc["v1"][row] < rc["v2"][row] else rc["p1"][row:row + 1]
            for k in range(2):
                d[k * nq:(k + 1) * nq] = row_grad(k, row, set(), other) - row_grad(k, row, set(), tgt[k][row:row + 1])
        return d
    return cands, delta


def policy_candidates(c, st, rp):
    """(candidates, delta) of the policy step from `st`: kinks of the policy and of both critics on (s, pi(s)), and with clipped
    double Q the rows whose two expected values tie"""
    nq = st["Q"].size // 2
    qn = [st["Q"][:nq], st["Q"][nq:]]
    p64 = st["P"]
    Oc, Op, A, NA, B = c.Oc, c.Op, c.A, c.NA, c.B
    s, cs = c.batch[0], c.cstates()
    z = _T(np.linspace(c.h["v_min"], c.h["v_max"], NA))

    def row_grad(row, flips, swap_min):
        Pp = _T(p64).requires_grad_(True)
        act_ = torch.tanh(_fwd_flip(Pp, Op, c.ph, A, _T(s[row:row + 1]), flips.get("pi", set())))
        xa = torch.cat([_T(cs[row:row + 1]), act_], dim=1)
        v = [(torch.softmax(_fwd_flip(_T(qn[k]), Oc + A, c.ch, NA, xa, flips.get(k, set())), dim=1) * z).sum() for k in range(2)]
        if c.clipped:
            first = bool(v[0] < v[1]) != swap_min
            q = v[0] if first else v[1]
        else:
            q = 0.5 * (v[0] + v[1])
        (-q / B).backward()
        return Pp.grad.numpy()
    xp = np.concatenate([cs, rp["actions"]], 1)
    pc = [(k_[0], "relu", "pi") + k_[1:] for k_ in _kinks(p64, Op, c.ph, s, KINK_TAU)]
    pc += [(k_[0], "relu", k) + k_[1:] for k in range(2) for k_ in _kinks(qn[k], Oc + A, c.ch, xp, KINK_TAU)]
    if c.clipped:
        lgs = [tw.critic_logits(_T(qn[k]), Oc, A, NA, _T(cs), _T(rp["actions"]), c.ch).numpy() for k in range(2)]
        sm = lambda lg: np.exp(lg - lg.max(1, keepdims=True)) / np.exp(lg - lg.max(1, keepdims=True)).sum(1, keepdims=True)
        vv = np.stack([sm(lg) @ z.numpy() for lg in lgs])
        tie = np.abs(vv[0] - vv[1]) / np.sqrt(0.5 * (vv ** 2).sum(0).mean())
        pc += [(float(tie[i]), "min", -1, int(i)) for i in np.nonzero(tie < KINK_TAU)[0]]

    def delta(cd):
        row = cd[3]
        if cd[1] == "min":
            return row_grad(row, {}, True) - row_grad(row, {}, False)
        return row_grad(row, {cd[2]: {(cd[4], cd[5])}}, False) - row_grad(row, {}, False)
    return pc, delta


def explain_step(c, st, rc, rp, gq_got, gp_got):
    """the twin's (critic, policy) gradients of the step from `st`, adjusted by at most MAX_FLIPS kink / tie candidates each towards
    the evaluated ones gq_got / gp_got (the gradients as they entered AdamW: after clip_grad_norm_)
    -> ((gq, taken, candidates, ratio before), (gp, taken, candidates, ratio before)), gq / gp before clipping"""
    out = []
    for got, ge, (cands, delta) in ((gq_got, np.concatenate([rc["g_q1"], rc["g_q2"]]), critic_candidates(c, st, rc)),
                                    (gp_got, rp["g_policy"], policy_candidates(c, st, rp))):
        sc = clip_scale(ge, c.h["max_grad_norm"])
        ga, taken = _explain(got / sc, ge, cands, delta, MAX_FLIPS)
        out.append((ga, taken, cands, _rel(got / sc, ge)))
    return out


def metric_floors(c):
    """floors only where a metric is a difference of larger terms (q_min / q_max and the policy loss, means of expected values over
    +- max|v|); q_loss and the gradient norms are held to 1e-5 of their own value"""
    qf = max(1.0, max(abs(c.h["v_min"]), abs(c.h["v_max"])) / 10.0)
    return np.array([0.0, qf, qf, 0.0]), np.array([qf, 0.0])


def _blocks(in_dim, hidden, out_dim):
    out, off, d = [], 0, in_dim
    for li, w in enumerate(list(hidden) + [out_dim]):
        out += [("W%d" % li, off, d * w), ("b%d" % li, off + d * w, w)]
        off += d * w + w
        d = w
    return out


def check_against_twin(c, r, st, eps, step, label=""):
    """a Run against the twin's two updates from `st`: every metric, every state vector; the gradients -- recovered from the first
    moments, (m - b1 m0) / (1 - b1) -- per vector and per parameter block, for an assignment of at most MAX_FLIPS kink / tie
    candidates per update.  -> ((ratio before flips, after, flips, candidates) for the critic and the policy update)"""
    rc, rp = c.steps(st, eps)
    gq_got = (r.out["qm"] - B1 * st["qm"]) / (1.0 - B1)
    gp_got = (r.out["pm"] - B1 * st["pm"]) / (1.0 - B1)
    (gq, tq, cq, rq0), (gp, tp, cp, rp0) = explain_step(c, st, rc, rp, gq_got, gp_got)
    new, cmet, pmet = c.apply(st, step, rc, rp, gq, gp)
    sq, sp = clip_scale(gq, c.h["max_grad_norm"]), clip_scale(gp, c.h["max_grad_norm"])
    res = ((rq0, _rel(gq_got, gq * sq), len(tq), len(cq)), (rp0, _rel(gp_got, gp * sp), len(tp), len(cp)))
    print(f"FastTD3 {label} (B={c.B}) step {step}: ||dg||/||g|| critic {rq0:.2e} -> {res[0][1]:.2e} with {len(tq)} of {len(cq)} kink / tie "
          f"candidates on their other side, policy {rp0:.2e} -> {res[1][1]:.2e} with {len(tp)} of {len(cp)}")
    cf, pf = metric_floors(c)
    bad = [("critic", i, r.cmetrics[i], cmet[i]) for i in range(4) if not abs(r.cmetrics[i] - cmet[i]) <= 1e-5 * max(abs(cmet[i]), cf[i])]
    bad += [("policy", i, r.pmetrics[i], pmet[i]) for i in range(2) if not abs(r.pmetrics[i] - pmet[i]) <= 1e-5 * max(abs(pmet[i]), pf[i])]
    # the first moments carry the gradient bar: m = b1 m0 + (1 - b1) g with m0 given, so ||dm|| = (1 - b1) ||dg||
    bad += [("g_critic", res[0][1])] if not res[0][1] < 1e-5 else []
    bad += [("g_policy", res[1][1])] if not res[1][1] < 1e-5 else []
    bad += [("flips", len(tq), len(tp))] if max(len(tq), len(tp)) > MAX_FLIPS else []
    nq = gq.size // 2
    for tag, got, ref, bl in [("q1", gq_got[:nq], gq[:nq] * sq, _blocks(c.Oc + c.A, c.ch, c.NA)), ("q2", gq_got[nq:], gq[nq:] * sq, _blocks(c.Oc + c.A, c.ch, c.NA)),
                              ("policy", gp_got, gp * sp, _blocks(c.Op, c.ph, c.A))]:
        bad += [(tag, name, _rel(got[o:o + n], ref[o:o + n])) for name, o, n in bl
                if not np.linalg.norm(got[o:o + n] - ref[o:o + n]) <= 2e-5 * np.linalg.norm(ref[o:o + n]) + 1e-12]
    bad += [(k, _rel(r.out[k], new[k])) for k in ("P", "Q", "QT") if not _rel(r.out[k], new[k]) < 1e-5]
    # the moments on what the step itself added -- m - b1 m0 = (1 - b1) g, v - b2 v0 = (1 - b2) g^2, with m0 / v0 given to both sides
    # (the whole vector after a first step): what the kernels computed
    for k, b, tol in (("pm", B1, 1e-5), ("qm", B1, 1e-5), ("pv", B2, 2e-5), ("qv", B2, 2e-5)):
        e = _rel(r.out[k] - b * st[k], new[k] - b * st[k])
        bad += [(k, e)] if not e < tol else []
    assert not bad, bad
    assert r.ccount == r.pcount == step
    return res, new


# ------------------------------------------------------------------------------------------------------------------ the cases
NAMES = ["narrow", "wide", "act64", "split3", "split_ragged", "many_rows", "head320"]


def shape_case(name, num_cus=256):
    """the case table of test_gpu_fasttd3_shapes.py.  num_cus only sizes many_rows (64 num_cus + 37 rows)"""
    c = {
        "narrow": lambda: Case(271, 5, 1, (64,), (64,), 2, 1, v_min=-3.0, v_max=7.0),
        "wide": lambda: Case(272, 48, 16, (1024, 64), (1024, 1024), 128, 333, clipped=False),
        "act64": lambda: Case(273, 70, 64, (128, 64, 64), (128, 64, 64), 65, 37, Op=33, Oc=29, max_grad_norm=0.05),
        "split3": lambda: Case(274, 48, 12, (256, 128, 64), (256, 128, 64), 51, 4099, clipped=False),
        "split_ragged": lambda: Case(275, 45, 17, (256, 128, 64), (256, 128, 64), 101, 4099),
        "many_rows": lambda: Case(276, 64, 64, (64,), (64,), 21, 64 * num_cus + 37, clipped=False),
        "head320": lambda: Case(277, 1, 1, (64, 320), (64, 320), 21, 13),
    }[name]()
    if name == "narrow":        # the one row: not done, a reward past v_max -- the projected target sits on the top atom
        c.batch[3][:] = 8.5
        c.batch[4][:] = 0.0
        c.batch[5][:] = 0.0
    return c


# ------------------------------------------------------------------------------------------------------------- the fp16 window
def fp16_window(c, st, eps):
    """what the split-operand engine's operands reach in the twin's two steps from `st`: max |weight|, max |activation| (every trunk
    GEMM's input rows; ReLU outputs are not bounded by a norm), max |d loss / d pre-activation| times bx_grad_scale(B) (the scaled
    per-sample gradient operand of the weight- and input-gradient GEMMs) -- to hold against 1023, 4094 and fp16's 65504"""
    from net_paths import bx_grad_scale
    trace = []
    c.steps(st, eps, trace=trace)
    seen = dict(act=max(float(x.detach().abs().max()) for x, _ in trace),
                grad=max(float(z.grad.abs().max()) for _, z in trace if z.grad is not None))
    return dict(weight=float(max(np.abs(st["P"]).max(), np.abs(st["Q"]).max(), np.abs(st["QT"]).max())), act=seen["act"],
                grad_scaled=seen["grad"] * bx_grad_scale(c.B))


# ------------------------------------------------------------------------------------------ a float32 evaluation on the CPU
def float32_flips(c, st, eps):
    """the explanation a plain float32 evaluation of both steps (the twin's dtype=np.float32: networks, projection, losses) needs
    against float64 -> explain_step's result"""
    rc, rp = c.steps(st, eps)
    rc32, rp32 = c.steps(st, eps, dtype=np.float32)
    g = lambda x: np.asarray(x, np.float64)
    sq = clip_scale(np.concatenate([rc["g_q1"], rc["g_q2"]]), c.h["max_grad_norm"])
    sp = clip_scale(rp["g_policy"], c.h["max_grad_norm"])
    return explain_step(c, st, rc, rp, g(np.concatenate([rc32["g_q1"], rc32["g_q2"]])) * sq, g(rp32["g_policy"]) * sp)
