"""Helpers shared by the FastSAC shape tests (test_fastsac_cases.py, test_gpu_fastsac_shapes.py): the library's hyperparameter
struct from a dict, a Case (a float64 oracle state of float32-representable values, a batch with terminations, truncations and
n-steps 1..4, noise per step), a Run (one rlx_fastsac_critic_update_f32 and one rlx_fastsac_policy_update_f32 call on device
copies of a state) and the comparison with its bars.

Both updates of a Run start from the SAME state: the policy update sees the critics and log_alpha from before the critic update,
so the oracle and the device get bit-identical float32 inputs in both, and each bar measures one update's kernels.

Bars (the ones test_gpu_fastsac.py holds the kernels to): gradients 1e-5 relative in L2 per vector (first step from zero moments:
g = m / (1 - b1)) and 2e-5 per parameter block; first moments 1e-5 (they are the gradient bar: m = b1 m0 + (1 - b1) g with m0
given); second moments 2e-5 (v is quadratic in g: twice the gradient bar); parameters, targets and log_alpha after the step 1e-6;
scalars 1e-5 relative; only the metrics that are differences of larger terms get a floor, the size of those terms: alpha
max(|entropy|, |target entropy|, 1) for the entropy loss (its square for the logged squared gradient), max(1, max|v| / 10) for the
policy loss (alpha log pi - q) and q_min / q_max."""
import numpy as np
import torch

from oracle import fastsac as ofs
from rlx_amd.hip import FastSacHparams, lnmlp_desc
from shape_batch import draw_batch, index_sets
from shape_batch import f32 as _f32

# learning_rate: AdamW's step lr g / (|g| + eps) has slope lr / eps where |g| is within eps = 1e-8 of zero, so the parameter bar
# (1e-6 of ||Q||) meets the absolute gradient noise on those few entries.  A plain float32 evaluation on the CPU
# (float32_critic_update: 2.9e-6 from the float64 gradient at 128 atoms, nearly all of it the float32 categorical projection)
# puts `wide`'s critics at 1.9e-6 and `dxlds`'s at 1.05e-6 with the reference's default 3e-4 -- the inputs, not a kernel, pass the
# bar -- and at a tenth of that with 3e-5.  test_fastsac_cases.py holds every case's float32 evaluation to half of each bar.
# weight_decay: AdamW's decay moves a parameter by the relative amount lr wd; 0.5 puts that at 1.5e-5, fifteen times the 1e-6 bar
# on P, Q, QT and log_alpha, so an update that dropped the (1 - lr wd) factor misses every one of them
# (test_fastsac_cases.py::test_the_bars_see_weight_decay).
HP = dict(gamma=0.97, tau=0.125, v_min=-20.0, v_max=20.0, log_std_min=-5.0, log_std_max=0.0, learning_rate=3e-5, weight_decay=0.5,
          adam_beta1=0.9, adam_beta2=0.95, target_entropy=-1.5, max_grad_norm=-1.0, log_alpha=float(np.log(0.05)))
CRITIC_KEYS = ("Q", "qm", "qv", "QT", "la", "am", "av")
POLICY_KEYS = ("P", "pm", "pv")
STATE_KEYS = POLICY_KEYS + CRITIC_KEYS


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


def _hp(h, nr_atoms, clipped):
    hp = FastSacHparams()
    for k in ("gamma", "tau", "v_min", "v_max", "log_std_min", "log_std_max", "target_entropy", "weight_decay"):
        setattr(hp, k, float(h[k]))
    hp.lr_policy = hp.lr_critic = hp.lr_alpha = float(h["learning_rate"])
    hp.adam_b1, hp.adam_b2, hp.adam_eps = float(h["adam_beta1"]), float(h["adam_beta2"]), 1e-8
    hp.nr_atoms, hp.clipped_double_q = int(nr_atoms), int(bool(clipped))
    hp.max_grad_norm = float(h.get("max_grad_norm", -1.0))
    return hp


class Case:
    """seeded per case.  O: the observation width, Op / Oc: the columns the policy / the critics see (index sets drawn from the
    seed; None: all of them -- then no critic_states are passed)"""

    def __init__(self, seed, O, A, policy_hidden, critic_hidden, NA, B, Op=None, Oc=None, clipped=False, **hp):
        self.h = dict(HP, **hp)
        rng = np.random.default_rng(seed)
        self.O, self.A, self.NA, self.B, self.clipped = O, A, NA, B, clipped
        self.ph, self.ch = tuple(policy_hidden), tuple(critic_hidden)
        self.pidx, self.cidx = index_sets(rng, O, Op, Oc)
        self.Op, self.Oc = (O if Op is None else Op), (O if Oc is None else Oc)
        self.split = self.pidx is not None or self.cidx is not None
        self.pd, self.qd = lnmlp_desc(self.Op, self.ph, 2 * A), lnmlp_desc(self.Oc + A, self.ch, NA)
        p, q = ofs.make_params(seed, self.Op, A, NA, self.Oc, self.ph, self.ch)
        p, q = p.astype(np.float64), [x.astype(np.float64) for x in q]
        zp, zq = np.zeros(p.size), np.zeros(2 * q[0].size)
        self.state = dict(P=p, pm=zp, pv=zp, Q=np.concatenate(q[:2]), qm=zq, qv=zq, QT=np.concatenate(q[2:]),
                          la=float(np.float32(self.h["log_alpha"])), am=0.0, av=0.0)
        self.scale = _f32(np.linspace(0.5, 1.5, A))
        self.batch, self.cbatch = draw_batch(rng, B, O, A, self.h, lambda z: np.tanh(z) * self.scale, self.pidx, self.cidx)   # the policy's columns, the critics'
        self.rng = rng

    def noise(self):
        return _f32(self.rng.standard_normal((self.B, self.A))), _f32(self.rng.standard_normal((self.B, self.A)))

    def kw(self):
        return dict(policy_hidden=self.ph, critic_hidden=self.ch)

    def twin(self, st, eps, step):
        """both updates from `st` (see the module docstring) -> (new state, critic metrics [8], policy metrics [3], (critic_step
        dict, policy_step dict))"""
        qp, qm, qv, qt, la, am, av, cmet, rc = ofs.critic_update(
            st["P"], st["Q"], st["qm"], st["qv"], st["QT"], st["la"], st["am"], st["av"], step, self.Oc, self.A, self.NA, self.batch, eps[0],
            self.scale, self.h, self.clipped, self.cbatch, **self.kw())
        pp, pm, pv, pmet, rp = ofs.policy_update(
            st["P"], st["pm"], st["pv"], step, st["Q"], st["la"], self.Oc, self.A, self.NA, self.batch[0], eps[1], self.scale, self.h,
            self.clipped, None if self.cbatch is None else self.cbatch[0], **self.kw())
        return dict(P=pp, pm=pm, pv=pv, Q=qp, qm=qm, qv=qv, QT=qt, la=la, am=am, av=av), cmet, pmet, (rc, rp)

    def run(self, ctx, dev, st, eps, step, key=(0, 7)):
        return Run(ctx, dev, self, st, eps, step, key)


class Run:
    """rlx_fastsac_critic_update_f32, then rlx_fastsac_policy_update_f32 against the critics and log_alpha from BEFORE it, on
    device copies of a state.  prof: ctx.prof_rows() of each update (taken when `profile`)."""

    def __init__(self, ctx, dev, c, st, eps, step, key=(0, 7), profile=False):
        d = {k: _t(np.atleast_1d(st[k]), dev) for k in STATE_KEYS}
        q0, la0 = d["Q"].clone(), d["la"].clone()
        hp = _hp(c.h, c.NA, c.clipped)
        batch = tuple(_t(x, dev) for x in c.batch)
        cb = (None, None) if c.cbatch is None else tuple(_t(x, dev) for x in c.cbatch)
        scale = _t(c.scale, dev)
        self.cmet, self.pmet = torch.zeros(8, device=dev), torch.zeros(3, device=dev)
        self.eps = (_t(eps[0], dev), _t(eps[1], dev))       # kept alive: the library holds the pointers
        self.prof = [None, None]
        ctx.dbg_set_sac_noise(*self.eps)
        try:
            if profile:
                ctx.prof_begin()
            self.key, self.ccount = ctx.fastsac_critic_update(c.pd, d["P"], c.qd, d["Q"], d["qm"], d["qv"], d["QT"], d["la"], d["am"], d["av"],
                                                              batch, scale, np.array(key, np.uint32), step - 1, hp, self.cmet,
                                                              critic_states=cb[0], critic_next_states=cb[1])
            if profile:
                ctx.prof_end()
                self.prof[0] = ctx.prof_rows()
                ctx.prof_begin()
            self.key, self.pcount = ctx.fastsac_policy_update(c.pd, d["P"], d["pm"], d["pv"], c.qd, q0, la0, batch[0], scale, self.key,
                                                              step - 1, hp, self.pmet, critic_states=cb[0])
            if profile:
                ctx.prof_end()
                self.prof[1] = ctx.prof_rows()
        finally:
            ctx.dbg_set_sac_noise(None, None)
        torch.cuda.synchronize()
        self.out = {k: d[k].cpu().numpy().astype(np.float64) for k in STATE_KEYS}
        for k in ("la", "am", "av"):
            self.out[k] = float(self.out[k][0])
        self.cmetrics, self.pmetrics = self.cmet.cpu().numpy().astype(np.float64), self.pmet.cpu().numpy().astype(np.float64)


def metric_floors(c, cmet):
    """floors only for the metrics that are differences of larger terms (entropy loss and its logged square, q_min / q_max, the
    policy loss); q_loss, entropy, the gradient norms and alpha are held to 1e-5 of their own value"""
    vmax = max(abs(c.h["v_min"]), abs(c.h["v_max"]))
    ent = cmet[7] * max(abs(cmet[4]), abs(c.h["target_entropy"]), 1.0)
    qf = max(1.0, vmax / 10.0)
    return np.array([0.0, ent, qf, qf, 0.0, 0.0, ent * ent, 0.0]), np.array([qf, 0.0, 0.0])


def check_metrics(c, r, cmet, pmet):
    cf, pf = metric_floors(c, cmet)
    bad = [("critic", i, r.cmetrics[i], cmet[i]) for i in range(8) if not abs(r.cmetrics[i] - cmet[i]) <= 1e-5 * max(abs(cmet[i]), cf[i])]
    bad += [("policy", i, r.pmetrics[i], pmet[i]) for i in range(3) if not abs(r.pmetrics[i] - pmet[i]) <= 1e-5 * max(abs(pmet[i]), pf[i])]
    assert not bad, bad


def _blocks_bad(got, ref, blocks, tag, tol=2e-5):
    return [(tag, name, float(np.linalg.norm(got[o:o + n] - ref[o:o + n]) / max(np.linalg.norm(ref[o:o + n]), 1e-30)))
            for name, o, n in blocks if not np.linalg.norm(got[o:o + n] - ref[o:o + n]) <= tol * np.linalg.norm(ref[o:o + n]) + 1e-12]


def gradient_ratios(c, r, rc, rp):
    """first step from zero moments: (critic, policy) ||dg|| / ||g|| of the gradients recovered from the first moments"""
    b1 = c.h["adam_beta1"]
    gq, _ = ofs.clip_grad_norm(np.concatenate([rc["g_q1"], rc["g_q2"]]), c.h["max_grad_norm"])
    gp, _ = ofs.clip_grad_norm(rp["g_policy"], c.h["max_grad_norm"])
    return (r.out["qm"] / (1.0 - b1), gq), (r.out["pm"] / (1.0 - b1), gp)


def check_against_twin(c, r, new, cmet, pmet, steps, first, old):
    """a Run against the oracle's two updates from the state `old`: every metric, every state vector; after a first step also the
    gradients per vector and per parameter block.  The moments are held to their bars on what the step itself added -- m - b1 m0 =
    (1 - b1) g, v - b2 v0 = (1 - b2) g^2, with m0 / v0 given to both sides -- which is the whole vector after a first step.
    -> (critic, policy) gradient error ratios (first step) or first-moment error ratios"""
    check_metrics(c, r, cmet, pmet)
    b1, b2 = c.h["adam_beta1"], c.h["adam_beta2"]
    bad = [(k, _rel(r.out[k], new[k])) for k in ("P", "Q", "QT") if not _rel(r.out[k], new[k]) < 1e-6]
    own = lambda k, b: (r.out[k] - b * np.asarray(old[k]), new[k] - b * np.asarray(old[k]))
    for k, b, tol in (("pm", b1, 1e-5), ("qm", b1, 1e-5), ("am", b1, 1e-5), ("pv", b2, 2e-5), ("qv", b2, 2e-5), ("av", b2, 2e-5)):
        if not _rel(*own(k, b)) < tol:
            bad.append((k, _rel(*own(k, b))))
    if not abs(r.out["la"] - new["la"]) <= 1e-6 * abs(new["la"]):
        bad.append(("la", r.out["la"], new["la"]))
    # log_alpha's own step (decay + AdamW, ~1e-4): within 1e-3 of it plus two float32 ulps of log_alpha
    la_step = new["la"] - old["la"]
    if not abs((r.out["la"] - old["la"]) - la_step) <= 1e-3 * abs(la_step) + 2.0 * float(np.spacing(np.float32(abs(new["la"])))):
        bad.append(("la step", r.out["la"] - old["la"], la_step))
    ratios = (_rel(*own("qm", b1)), _rel(*own("pm", b1)))
    if first:
        (gq_d, gq), (gp_d, gp) = gradient_ratios(c, r, *steps)
        ratios = (_rel(gq_d, gq), _rel(gp_d, gp))
        bad += [("g_critic", ratios[0])] if not ratios[0] < 1e-5 else []
        bad += [("g_policy", ratios[1])] if not ratios[1] < 1e-5 else []
        nq = gq.size // 2
        qb = ofs.blocks(c.Oc + c.A, c.ch, c.NA)
        for k in range(2):
            bad += _blocks_bad(gq_d[k * nq:(k + 1) * nq], gq[k * nq:(k + 1) * nq], qb, "q%d" % (k + 1))
        bad += _blocks_bad(gp_d, gp, ofs.blocks(c.Op, c.ph, 2 * c.A), "policy")
    assert not bad, bad
    assert r.ccount == r.pcount == (1 if first else 2)
    return ratios


# ------------------------------------------------------------------------------------------ a float32 evaluation on the CPU
def _steps(c, st, eps, **kw):
    """the oracle's (critic_step, policy_step) from `st`; kw: critic_step's dtype= / both steps' trace="""
    nq = st["Q"].size // 2
    q = [st["Q"][:nq], st["Q"][nq:], st["QT"][:nq], st["QT"][nq:]]
    rc = ofs.critic_step(st["P"], *q, st["la"], c.Oc, c.A, c.NA, c.batch, eps[0], c.scale, c.h, c.clipped, c.cbatch, **c.kw(), **kw)
    kw.pop("dtype", None)
    rp = ofs.policy_step(st["P"], q[0], q[1], st["la"], c.Oc, c.A, c.NA, c.batch[0], eps[1], c.scale, c.h, c.clipped,
                         None if c.cbatch is None else c.cbatch[0], **c.kw(), **kw)
    return rc, rp


def float32_critic_update(c, st, eps, step=1):
    """the critic update from `st` with oracle.fastsac.critic_step evaluated in plain float32 (torch on the CPU: the networks, the
    sampled next action, the categorical projection and the loss; AdamW applied to that gradient in float64) -> (gradient
    [q1 | q2] after clip_grad_norm_, critics after the step).  What float32 alone costs against the float64 oracle: at 128 atoms the
    projection's bin position (tz - v_min) / dz lies in [0, 127] and carries ~64 ulp, which lands as an absolute error of a few
    1e-6 in the interpolation weights of every target row"""
    nq = st["Q"].size // 2
    rc = ofs.critic_step(st["P"], st["Q"][:nq], st["Q"][nq:], st["QT"][:nq], st["QT"][nq:], st["la"], c.Oc, c.A, c.NA, c.batch, eps[0],
                         c.scale, c.h, c.clipped, c.cbatch, dtype=np.float32, **c.kw())
    gq, _ = ofs.clip_grad_norm(np.concatenate([rc["g_q1"], rc["g_q2"]]).astype(np.float64), c.h["max_grad_norm"])
    qp, _, _ = ofs.adamw(np.asarray(st["Q"], np.float64), gq, st["qm"], st["qv"], step, c.h["learning_rate"], c.h["weight_decay"],
                         c.h["adam_beta1"], c.h["adam_beta2"])
    return gq, qp


# ------------------------------------------------------------------------------------------------------------- the fp16 window
def fp16_window(c, st, eps, step=1):
    """what the split-operand engine's operands reach in the oracle's two steps from `st` (their trace= hook): max |weight|, max
    |activation| (every trunk GEMM's input rows), max |d loss / d pre-norm value| times bx_grad_scale(B) (the scaled per-sample
    gradient operand of the weight- and input-gradient GEMMs) -- to hold against 1023, 4094 and fp16's 65504 (gemm_bx.h)"""
    from net_paths import bx_grad_scale
    seen = dict(act=0.0, grad=0.0)
    trace = []
    _steps(c, st, eps, trace=trace)
    for x, *layers in trace:
        seen["act"] = max([seen["act"], float(x.detach().abs().max())] + [float(h.detach().abs().max()) for _, h in layers[:-1]])
        seen["grad"] = max([seen["grad"]] + [float(z.grad.abs().max()) for z, _ in layers if z.grad is not None])
    return dict(weight=float(max(np.abs(st["P"]).max(), np.abs(st["Q"]).max(), np.abs(st["QT"]).max())), act=seen["act"],
                grad_scaled=seen["grad"] * bx_grad_scale(c.B))


# ------------------------------------------------------------------------------------------------------------------ the cases
NAMES = ["narrow", "wide", "act65", "dxlds", "split4", "split_ragged", "many_rows"]


def shape_case(name, num_cus=256):
    """the case table of test_gpu_fastsac_shapes.py.  num_cus only sizes many_rows (64 num_cus + 37 rows)"""
    c = {
        "narrow": lambda: Case(171, 5, 1, (64,), (64,), 2, 1, clipped=True, v_min=-3.0, v_max=7.0),
        "wide": lambda: Case(172, 48, 12, (768, 704), (768, 768), 128, 333),
        "act65": lambda: Case(173, 70, 65, (128, 64, 64, 64), (128, 64, 64, 64), 65, 37, Op=33, Oc=29, clipped=True, max_grad_norm=0.05),
        "dxlds": lambda: Case(174, 45, 27, (256, 128), (768, 192), 51, 130, clipped=True),
        "split4": lambda: Case(175, 48, 4, (128, 64, 64, 64), (128, 64, 64, 64), 51, 4099),
        "split_ragged": lambda: Case(176, 45, 17, (256, 128), (256, 128), 101, 4099, clipped=True),
        "many_rows": lambda: Case(177, 64, 40, (64,), (64,), 21, 64 * num_cus + 37),
    }[name]()
    if name == "narrow":        # the one row: not done, a reward past v_max -- every projected target sits on the top atom
        c.batch[3][:] = 8.5
        c.batch[4][:] = 0.0
        c.batch[5][:] = 0.0
    return c
