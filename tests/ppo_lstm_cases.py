"""Helpers shared by the recurrent-PPO shape tests (test_ppo_lstm_cases.py, test_gpu_ppo_lstm_shapes.py): the case table of the sequence
minibatch pass (rlx_ppo_lstm_minibatch_fwd_bwd_f32), of the whole update (rlx_ppo_lstm_update_f32) and of the acting step
(rlx_ppo_lstm_act_f32) over the shapes check_lstm_desc accepts (net_paths.lstm_check_desc restates its clauses).

A Case holds seeded float32 parameters and a rollout built the way test_gpu_ppo_lstm.py builds them (ol.init_params plus a 0.03
perturbation, the "B" critic, old log-probs from the oracle plus 0.05 noise), ne env indices of N, the float64 autograd result
(oracle/ppo_lstm.py: ppo_lstm_loss), computed once and shared by every test and option setting, and what the selection mirror
(net_paths.ppo_lstm_pass) says the pass must run.

Bars (test_gpu_ppo_lstm.py's): policy-gradient loss rel 1e-5 / abs 1e-6, critic and entropy loss rel 1e-5, KL rel 1e-4 / abs 2e-8, clip
fraction 2 / (T ne); per parameter block max error <= 5e-5 block scale + 1e-7 and L2 <= 1e-5 ||ref|| + 1e-9; whole policy and whole
critic gradient L2-relative < 1e-5."""
import functools

import numpy as np

import net_paths as npth
from oracle import nets, ppo as oppo, ppo_lstm as ol, prng

CLIP, ENT, VF = 0.2, 0.01, 0.5
ADAM_EPS = 1e-5
GRAD_BAR = 1e-5
RATIO_MARGIN = 1e-5          # no probability ratio of a case within this of 1 +- CLIP: the clip indicator is the same in any precision
METRICS = (("loss/policy_gradient_loss", 1e-5, 1e-6), ("loss/critic_loss", 1e-5, 0.0), ("loss/entropy_loss", 1e-5, 0.0),
           ("policy_ratio/approx_kl", 1e-4, 2e-8))
LR, UPD_EPOCHS, OPT_COUNT0 = 3e-4, 2, 3          # the trajectory cases: N = 2 ne, two epochs = four updates, three earlier Adam steps

_f64 = lambda a: np.asarray(a, np.float64)


def _torch():
    import torch
    return torch


def rel(got, exp):
    return float(np.linalg.norm(_f64(got) - exp) / max(np.linalg.norm(exp), 1e-30))


def make_nets(O, A, E, torso, share, cell, combine, rng, perturb=0.03, critic=None, std_dev=1.0):
    """test_gpu_ppo_lstm.py's _setup at any shape -> (policy spec, float32 parameters, critic spec, float32 parameters)"""
    spec = ol.LstmPolicySpec(O, A, E, npth.LSTM_H, tuple(torso), share, cell, combine)
    p = ol.init_params(spec, rng, std_dev)
    p = (p + perturb * rng.standard_normal(p.shape)).astype(np.float32)
    cs = critic or nets.make_spec("B", O, 1, False)
    cp = nets.init_params(cs, rng, 1.0)
    cp = (cp + perturb * rng.standard_normal(cp.shape)).astype(np.float32)
    return spec, p, cs, cp


def make_rollout(spec, p, T, N, rng, p_done=0.15, p_far=0.25, act_scale=1.0):
    """test_gpu_ppo_lstm.py's _rollout_case -> (states, actions, old log-probs, returns, advantages, dones, c0, h0).  On top of its
    0.05 noise a quarter of the old log-probs is moved by +-0.35, well past the clip range of 0.2 (the noise alone leaves a ratio
    beyond 1 +- 0.2 once in 10^4 rows: the clipped branch of the loss and the clip fraction would not be exercised)"""
    torch = _torch()
    O, A = spec.O, spec.A
    states = rng.standard_normal((T, N, O)).astype(np.float32)
    actions = (act_scale * rng.standard_normal((T, N, A))).astype(np.float32)
    dones = (rng.random((T, N)) < p_done).astype(np.float32)
    c0 = (0.5 * rng.standard_normal((N, spec.H))).astype(np.float32)
    h0 = np.tanh(0.5 * rng.standard_normal((N, spec.H))).astype(np.float32)
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    with torch.no_grad():
        mean = ol.forward_sequence(spec, t64(p), t64(states), t64(dones), t64(c0), t64(h0)).numpy()
    logstd = p[spec.off["logstd"][0]:][:A].astype(np.float64)[None, None, :]
    logp = ((-0.5 * ((actions - mean) / np.exp(logstd)) ** 2 - 0.5 * ol.LOG_2PI - logstd).sum(-1)
            + 0.05 * rng.standard_normal((T, N)) + 0.35 * (rng.random((T, N)) < p_far) * rng.choice([-1.0, 1.0], (T, N))).astype(np.float32)
    returns = rng.standard_normal((T, N)).astype(np.float32)
    adv = (rng.standard_normal((T, N)) * 2 + 0.3).astype(np.float32)
    return states, actions, logp, returns, adv, dones, c0, h0


def loss_and_grads(spec, p, cs, cp, rollout, env_idx, dtype):
    """the oracle's loss on the minibatch of env columns env_idx, evaluated in `dtype` (advantages normalised over the minibatch in
    `dtype` too) -> (metrics dict of floats, policy gradient, critic gradient, probability ratios [T, ne])"""
    torch = _torch()
    states, actions, logp, returns, adv, dones, c0, h0 = rollout
    td = torch.float64 if dtype == np.float64 else torch.float32
    t = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, dtype=dtype)), dtype=td)
    P, C = t(p).requires_grad_(True), t(cp).requires_grad_(True)
    a = oppo.normalize_advantages(adv[:, env_idx].astype(dtype))
    seq = (t(states[:, env_idx]), t(actions[:, env_idx]), t(logp[:, env_idx]), t(returns[:, env_idx]), t(a), t(dones[:, env_idx]),
           t(c0[env_idx]), t(h0[env_idx]))
    loss, met = ol.ppo_lstm_loss(spec, P, cs, C, *seq, CLIP, ENT, VF)
    loss.backward()
    with torch.no_grad():
        mean = ol.forward_sequence(spec, P.detach(), seq[0], seq[5], seq[6], seq[7])
        logstd = spec.get(P.detach(), "logstd")[None, None, :]
        nlp = (-0.5 * ((seq[1] - mean) / torch.exp(logstd)) ** 2 - 0.5 * ol.LOG_2PI - logstd).sum(-1)
        ratio = torch.exp(nlp - seq[2]).numpy().astype(np.float64)
    return {k: float(v.detach()) for k, v in met.items()}, P.grad.numpy(), C.grad.numpy(), ratio


def compare(spec, T, ne, oracle, met, gp, gc):
    """device metrics [>= 5] and flat gradients against a float64 oracle result -> ({metric: (got, expected, allowed)},
    {policy block: (max error, allowed, L2 error, allowed)}, {"policy" / "critic": ||dg|| / ||g||}); nothing is asserted here"""
    met_e, gp_e, gc_e = oracle[:3]
    m, gp, gc = _f64(met), _f64(gp), _f64(gc)
    rows = {name: (m[i], met_e[name], atol + rtol * abs(met_e[name])) for i, (name, rtol, atol) in enumerate(METRICS)}
    rows["policy_ratio/clip_fraction"] = (m[4], met_e["policy_ratio/clip_fraction"], 2.0 / (T * ne))
    blocks = {}
    for name, (o, n) in spec.off.items():
        ref = gp_e[o:o + n]
        blocks[name] = (float(np.abs(gp[o:o + n] - ref).max()), 5e-5 * max(float(np.abs(ref).max()), 1e-6) + 1e-7,
                        float(np.linalg.norm(gp[o:o + n] - ref)), 1e-5 * float(np.linalg.norm(ref)) + 1e-9)
    return rows, blocks, {"policy": rel(gp, gp_e), "critic": rel(gc, gc_e)}


def assert_within(rows, blocks, whole, fraction=1.0):
    """every figure of compare() within `fraction` of its bar"""
    for k, (got, exp, allowed) in rows.items():
        assert abs(got - exp) <= fraction * allowed, (k, got, exp, allowed)
    for k, (emax, amax, el2, al2) in blocks.items():
        assert emax <= fraction * amax, (k, "max", emax, amax)
        assert el2 <= fraction * al2, (k, "L2", el2, al2)
    for k, v in whole.items():
        assert v < fraction * GRAD_BAR, (k, v)


class Case:
    def __init__(self, name, O, A, E, torso, T, N, ne, cell="lstm", combine="concat", share=False, seed=0, std_dev=1.0, act_scale=1.0):
        self.std_dev, self.act_scale = std_dev, act_scale
        self.name, self.O, self.A, self.E, self.torso, self.T, self.N, self.ne = name, O, A, E, tuple(torso), T, N, ne
        self.cell, self.combine, self.share, self.seed = cell, combine, bool(share), seed
        self._built = False

    @property
    def desc_args(self):
        """(O, A, E, H, torso, cell, combine) as check_lstm_desc and its mirror read them"""
        return (self.O, self.A, self.E, npth.LSTM_H, self.torso, npth.CELL_GRU if self.cell == "gru" else npth.CELL_LSTM,
                npth.COMBINE_FILM if self.combine == "film" else npth.COMBINE_CONCAT)

    def expect(self, options=None):
        return npth.ppo_lstm_pass(self.O, self.A, self.E, self.torso, self.share, self.cell == "gru", self.combine == "film", self.T, self.ne,
                                  options=options)

    def build(self):
        if self._built:
            return self
        rng = np.random.default_rng(20261021 + self.seed)
        self.spec, self.p, self.cs, self.cp = make_nets(self.O, self.A, self.E, self.torso, self.share, self.cell, self.combine, rng,
                                                           std_dev=self.std_dev)
        self.rollout = make_rollout(self.spec, self.p, self.T, self.N, rng, act_scale=self.act_scale)
        self.env_idx = rng.permutation(self.N)[:self.ne].astype(np.int32)
        self._built = True
        return self

    def evaluate(self, dtype):
        c = self.build()
        return loss_and_grads(c.spec, c.p, c.cs, c.cp, c.rollout, c.env_idx, dtype)

    @functools.cached_property
    def oracle(self):
        """(metrics, policy gradient, critic gradient, ratios) in float64: computed once per case"""
        return self.evaluate(np.float64)


class UpdateCase:
    """The whole update on a base case's network: T steps of N = 2 ne environments, two epochs = four updates of T ne rows, from
    opt_count = 3 with non-zero Adam moments, max_grad_norm at half the smaller gradient norm of the first update (clipping acts)."""

    def __init__(self, base):
        self.base, self.name = base, base.name
        self.T, self.ne, self.N = base.T, base.ne, 2 * base.ne
        self._built = False

    def build(self):
        if self._built:
            return self
        b = self.base.build()
        rng = np.random.default_rng(20271021 + b.seed)
        self.spec, self.cs, self.p, self.cp = b.spec, b.cs, b.p, b.cp
        self.rollout = make_rollout(b.spec, b.p, self.T, self.N, rng)
        self.pm, self.cm = ((0.01 * rng.standard_normal(x.shape)).astype(np.float32) for x in (b.p, b.cp))
        self.pv, self.cv = (((0.01 * rng.standard_normal(x.shape)) ** 2 + 1e-8).astype(np.float32) for x in (b.p, b.cp))
        self.key = prng.prng_key(9 + b.seed)
        self.n_upd = UPD_EPOCHS * (self.N // self.ne)
        self.key_out, self.idx = ol.env_minibatch_indices(self.key, self.N, UPD_EPOCHS, self.N // self.ne, self.ne)
        _, gp, gc, _ = loss_and_grads(self.spec, self.p, self.cs, self.cp, self.rollout, self.idx[0], np.float64)
        self.max_grad_norm = float(np.float32(0.5 * min(np.linalg.norm(gp), np.linalg.norm(gc))))
        self._built = True
        return self

    def trajectory(self, grad_dtype):
        """the oracle loop of test_gpu_ppo_lstm.py (gradients by autograd in grad_dtype, float32 optimizer state like the device's)
        -> ([per update: metrics dict + the two gradient norms], policy parameters, critic parameters)"""
        c = self.build()
        po, co, pm, pv, cm, cv = c.p.copy(), c.cp.copy(), c.pm.copy(), c.pv.copy(), c.cm.copy(), c.cv.copy()
        out = []
        for u in range(c.n_upd):
            met, gp, gc, _ = loss_and_grads(c.spec, po, c.cs, co, c.rollout, c.idx[u], grad_dtype)
            gp, n_p = oppo.clip_by_global_norm(gp.astype(np.float32), c.max_grad_norm)
            gc, n_c = oppo.clip_by_global_norm(gc.astype(np.float32), c.max_grad_norm)
            met["gradients/policy_grad_norm"], met["gradients/critic_grad_norm"] = float(n_p), float(n_c)
            out.append(met)
            po, pm, pv = oppo.adam_step(po, gp, pm, pv, OPT_COUNT0 + u, LR, eps=ADAM_EPS)
            co, cm, cv = oppo.adam_step(co, gc, cm, cv, OPT_COUNT0 + u, LR, eps=ADAM_EPS)
        return out, po, co

    @functools.cached_property
    def trajectory64(self):
        return self.trajectory(np.float64)


def _both_cells(name, *args, seeds=(0, 0), **kw):
    return [Case(f"{name}-{cell}", *args, cell=cell, seed=s, **kw) for cell, s in zip(("lstm", "gru"), seeds)]


# name, O, A, E, torso, T, N, ne: the issue's table, what each reaches next to it
_SMALL = (
    # minimum of every width; head on the LDS-staged kernel with K = 4; a second row tile with 1 valid env
    _both_cells("min", 1, 1, 64, (64, 4, 4), 2, 20, 17)
    # maximum widths; one exactly full 16-env tile; odd T.  (64 actions at unit std and unit spread have log-probs near -91, which any
    #  fp32 sum of 64 terms knows to 4e-6 a row: over 48 rows that alone is the 1e-6 the policy-gradient loss is allowed, and half the
    #  gradient's 1e-5 -- the float32 oracle shows both.  std 0.4 = exp(-0.5 log 2 pi) and actions within half a std keep them near -10.)
    + _both_cells("max", 32, 64, 512, (512, 8, 12), 3, 16, 16, std_dev=0.4, act_scale=0.2)
    # shared encoder wider than the first torso layer: d obs_latent [M, E] does not fit a slot of M torso[0] floats
    + _both_cells("share_concat", 6, 3, 256, (64, 4, 4), 4, 30, 24, share=True)
    # ... the same on the FiLM branch; GB of width 2 E; three tiles, the last with 1 env
    + _both_cells("share_film", 9, 2, 128, (64, 8, 8), 4, 40, 33, share=True, combine="film")
    # FiLM GEMM with N = 1024; widths that are no multiples of 64 or 128; A > 8
    + _both_cells("film_wide", 7, 9, 512, (128, 132, 68), 5, 18, 15, combine="film")
    # a single step through the two-step-unrolled sequence kernels
    + _both_cells("t1_ne1", 17, 6, 192, (320, 256, 128), 1, 3, 1)
    + _both_cells("t1_ne31", 17, 6, 192, (320, 256, 128), 1, 33, 31)
)
# the recurrent product on the exact-fp32 MFMA (k_lstm_seq_fwd / bwd <*, false>): by gemm_bx = 0 and by bx_debug & 256, on a launch of
# full tiles (<true, false>) and on a ragged one (<false, false>).  The inputs are the base case's: one oracle evaluation serves all.
_EXACT = [(base, label, opts) for base in ("max-lstm", "min-lstm") for label, opts in (("gemm_bx0", {"gemm_bx": 0}), ("bx_debug256", {"bx_debug": 256}))]
# 4096 rows and above: the split-operand engine prepares t1, t2, t3 and Wi
_BIG = [
    Case("big_full", 17, 6, 64, (256, 128, 64), 16, 260, 256, cell="lstm"),                # K1 = 128; full tiles; exactly 4096 rows
    Case("big_ragged", 17, 6, 192, (320, 132, 68), 8, 523, 520, cell="gru", combine="film", share=True),   # K1 = 192 on FiLM; ragged widths; an 8-env tail tile; 4160 rows
]
_TABLE = list(_SMALL) + _BIG
for _i, _c in enumerate(_TABLE):
    _c.seed += 100 * _i
CASES = {c.name: c for c in _TABLE}
NAMES = tuple(CASES)
# (case name, label, options) of every run of the minibatch test
RUNS = [(c.name, "defaults", {}) for c in _TABLE] + _EXACT
UPDATE_NAMES = ("share_concat-lstm", "share_film-lstm", "min-lstm", "share_concat-gru")
UPDATES = {n: UpdateCase(CASES[n]) for n in UPDATE_NAMES}


def case(name):
    return CASES[name].build()


def run_options(name, label):
    return next(o for n, l, o in RUNS if n == name and l == label)


# ---- refusals: one case per clause of check_lstm_desc -> name: (O, A, E, H, torso, cell, combine)
_OK = dict(O=5, A=3, E=64, H=64, torso=(64, 8, 8), cell=npth.CELL_LSTM, combine=npth.COMBINE_CONCAT)


def _refused(**kw):
    d = dict(_OK, **kw)
    return (d["O"], d["A"], d["E"], d["H"], tuple(d["torso"]), d["cell"], d["combine"])


REFUSED = {
    "obs_0": _refused(O=0), "obs_33": _refused(O=33), "hidden_128": _refused(H=128), "enc_96": _refused(E=96), "enc_576": _refused(E=576),
    "torso0_96": _refused(torso=(96, 8, 8)), "torso0_576": _refused(torso=(576, 8, 8)), "torso1_6": _refused(torso=(64, 6, 8)),
    "torso2_0": _refused(torso=(64, 8, 0)), "act_0": _refused(A=0), "act_65": _refused(A=65), "cell_2": _refused(cell=2),
    "combine_2": _refused(combine=2),
    # 0 and negative multiples pass `% 64 == 0` and `% 4 == 0`: each width has a lower bound of its own
    "torso0_0": _refused(torso=(0, 8, 8)), "torso0_neg64": _refused(torso=(-64, 8, 8)), "torso1_0": _refused(torso=(64, 0, 8)),
    "torso1_neg64": _refused(torso=(64, -64, 8)), "torso2_neg64": _refused(torso=(64, 8, -64)), "enc_0": _refused(E=0),
}
# the field each refusal's message must name
REFUSED_FIELD = {"obs": "obs_dim", "hidden": "lstm_hidden_dim", "enc": "obs_encoding_dim", "torso0": "torso[0]", "torso1": "torso[1]",
                 "torso2": "torso[2]", "act": "act_dim", "cell": "cell", "combine": "combine"}
AFTER_REFUSAL = "share_film-lstm"       # the small accepted case the context must serve correctly after each refusal


# ---- the acting step
class ActCase:
    """one acting step of n envs: test_gpu_ppo_lstm.py's _act_case at any shape, with the float64 oracle's carry, action, log-prob,
    value and processed action"""

    def __init__(self, E, torso, A, O, n, cell, combine="concat", share=False, critic=None, seed=0):
        torch = _torch()
        rng = np.random.default_rng(20281021 + seed)
        self.n, self.A, self.O = n, A, O
        self.spec, self.p, self.cs, self.cp = make_nets(O, A, E, torso, share, cell, combine, rng, critic=critic)
        self.obs = rng.standard_normal((n, O)).astype(np.float32)
        self.cobs = None if critic is None else rng.standard_normal((n, critic.in_dim)).astype(np.float32)
        self.c = (0.5 * rng.standard_normal((n, npth.LSTM_H))).astype(np.float32)
        self.h = np.tanh(0.5 * rng.standard_normal((n, npth.LSTM_H))).astype(np.float32)
        self.key = prng.prng_key(11 + n + seed)
        self.lo, self.hi = np.full(A, -2.0, np.float32), np.full(A, 3.0, np.float32)
        t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
        with torch.no_grad():
            mean, c2, h2 = ol.apply_one_step(self.spec, t64(self.p), t64(self.obs), t64(self.c), t64(self.h))
        ks = prng.split(self.key, 2)
        eps = prng.normal(ks[1], (n, A))
        logstd = self.p[self.spec.off["logstd"][0]:][:A].astype(np.float64)
        self.key_out = ks[0]
        self.c2, self.h2 = c2.numpy(), h2.numpy()
        self.action = mean.numpy() + np.exp(logstd) * eps
        self.logp = oppo.gaussian_log_prob(self.action, mean.numpy(), logstd[None, :])
        val, _ = nets.forward(self.cs, self.cp.astype(np.float64), (self.obs if self.cobs is None else self.cobs).astype(np.float64))
        self.value = val[:, 0]
        self.processed = -2.0 + 0.5 * (np.clip(self.action, -1, 1) + 1.0) * 5.0

    def fused(self, fused_recurrent_act=1):
        s = self.spec
        return npth.lstm_act_fused(s.E, s.torso, s.A, s.combine == "film", self.cs.in_dim, tuple(self.cs.hidden), fused_recurrent_act)


# _act_case's bars: name -> (rtol, atol)
ACT_BARS = dict(c=(1e-5, 2e-6), h=(1e-5, 2e-6), action=(1e-5, 1e-5), logp=(1e-5, 2e-5), value=(1e-5, 5e-6), processed=(1e-5, 1e-5))
# the corners of the fused decoder's envelope (rollout_decoder_supported): K0 = E + 64 in {128, 256}, every admitted torso pattern
ACT_E, ACT_TORSO, ACT_A, ACT_O, ACT_N = (64, 192), ((256, 128, 256), (512, 256, 128), (256, 256, 256)), (1, 32), (1, 32), (1, 31, 33, 65)
# just outside it: what -> (E, torso, A, combine); each must take the generic path
ACT_OUTSIDE = {"enc_256": (256, (512, 256, 128), 6, "concat"), "act_33": (64, (512, 256, 128), 33, "concat"),
               "torso0_64": (64, (64, 256, 128), 6, "concat"), "torso1_132": (64, (512, 132, 128), 6, "concat"),
               "film": (64, (512, 256, 128), 6, "film")}
