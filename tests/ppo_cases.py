"""Helpers shared by the PPO shape tests (test_ppo_cases.py, test_gpu_ppo_shapes.py) and test_gpu_bench_shapes.py: the case table
of the minibatch pass (rlx_ppo_minibatch_fwd_bwd_f32) and of the whole update (rlx_ppo_update_f32) over the shapes the library's
checks accept from 4096 rows on, where the split-operand engine and its specialised kernels take over.

A Case holds seeded float32 parameters and a pool of 2 mb rows built the way test_gpu_bench_shapes.py builds them (nets.MLPSpec
directly, init_params plus a 0.05 perturbation, old log-probs from the oracle plus noise), the mb gathered row indices, the float64
oracle result (oracle/ppo.py: ppo_loss_and_grads), computed once and shared by every test and twin setting, and what the selection
mirror (net_paths.ppo_pass) says the pass must run.

Bars (test_gpu_bench_shapes.py's): losses and their combination rtol 1e-5 / atol 1e-6, KL rtol 1e-5 / atol 1e-7, clip fraction
1.5 / mb, ||dg|| / ||g|| < 1e-5 per network and per parameter block."""
import functools

import numpy as np

import net_paths as npth
from oracle import nets, ppo as oppo

KINK = 8e-6      # |z| / rms below which an fp32 evaluation of a 256-term dot product may land on either side of zero (K eps / 4)
CLIP, ENT, CC = 0.1, 0.01, 0.7
GRAD_BAR = 1e-5
METRICS = (("loss/policy_gradient_loss", 1e-5, 1e-6), ("loss/critic_loss", 1e-5, 1e-6), ("loss/entropy_loss", 1e-5, 1e-6),
           ("policy_ratio/approx_kl", 1e-5, 1e-7))
LR, UPD_EPOCHS = 3e-4, 2                     # the trajectory cases: T = 2, N = mb, two epochs = four updates of mb rows
# (mid: the twin schedule chosen by size; wide33 / wide105: rows gathered at a padded stride by the whole-update entries -- the record
#  gather at 64 and 128 floats per record, the grouped buffers' offsets)
UPDATE_NAMES = ("h2_512", "act9", "flax256", "mid", "wide33", "wide105")
DIST_NAMES = ("wide33", "wide105")           # ... and through rlx_ppo_update_dist_f32 as the one rank that holds every row

_f64 = lambda a: np.asarray(a, np.float64)


def kink_entries(spec, params, x, tau):
    """(layer, row, unit, |z| / rms) of every ReLU pre-activation of the batch within tau of zero, relative to the row's RMS
    pre-activation (float64): a unit within fp32 rounding (a few 1e-7 relative for a 256-term fp32 dot product) of its kink has an
    UNDEFINED fp32 gradient -- any fp32 evaluation may land on either side."""
    h, out = x.astype(np.float64), []
    for li, L in enumerate(spec.layers):
        z = h @ params[L["W"]:L["W"] + L["in"] * L["out"]].reshape(L["in"], L["out"]) + params[L["b"]:L["b"] + L["out"]]
        m = np.abs(z) / np.sqrt((z * z).mean(axis=1, keepdims=True))
        out += [(li, int(i), int(j), float(m[i, j])) for i, j in zip(*np.nonzero(m < tau))]
        h = np.maximum(z, 0.0)
    return out


def blocks(spec):
    """(name, offset, length) of every parameter block of the flat layout."""
    out = []
    for li, L in enumerate(spec.layers):
        out.append((f"W{li}", L["W"], L["in"] * L["out"]))
        out.append((f"b{li}", L["b"], L["out"]))
        if "g" in L:
            out.append((f"ln_scale{li}", L["g"], L["out"]))
            out.append((f"ln_bias{li}", L["be"], L["out"]))
    out.append(("Wh", spec.head["W"], spec.head["in"] * spec.head["out"]))
    out.append(("bh", spec.head["b"], spec.head["out"]))
    if spec.has_logstd:
        out.append(("logstd", spec.logstd, spec.out_dim))
    return out


def rel(got, exp):
    return float(np.linalg.norm(_f64(got) - exp) / max(np.linalg.norm(exp), 1e-30))


class Case:
    def __init__(self, name, O, hidden, A, mb, act=nets.ACT_ELU, ln=True, seed=None, defaults=False):
        """defaults: run at the library's default options (otherwise at ppo_twin 0, and at 1 as well)"""
        self.name, self.O, self.hidden, self.A, self.mb, self.act, self.ln = name, O, tuple(hidden), A, mb, act, bool(ln)
        self.seed, self.defaults = seed, defaults
        self.shape = (O, self.hidden, A, act, self.ln, mb)
        self.ps, self.cs = nets.MLPSpec(O, hidden, A, act, ln, True), nets.MLPSpec(O, hidden, 1, act, ln, False)
        self._built = False

    # ---- what the pass must run
    def settings(self):
        """[(label, options the test sets, options the mirror is asked with)]"""
        if self.defaults:        # rlx_ppo_minibatch_fwd_bwd_f32 takes the twin pass only when it is forced: the default is two chains
            return [("defaults", {}, {})]
        return [("twin0", {"ppo_twin": 0}, {"ppo_twin": 0}), ("twin1", {"ppo_twin": 1}, {"ppo_twin": 1})]

    def expect(self, mirror_opts):
        return npth.ppo_pass(*self.shape, mirror_opts)

    # ---- inputs
    def build(self):
        if self._built:
            return self
        O, A, mb, ps, cs = self.O, self.A, self.mb, self.ps, self.cs
        B = 2 * mb
        rng = np.random.default_rng(20261021 + self.seed)
        self.pp = (nets.init_params(ps, rng, 0.01) + 0.05 * rng.standard_normal(ps.n_params)).astype(np.float32)
        self.cp = (nets.init_params(cs, rng, 1.0) + 0.05 * rng.standard_normal(cs.n_params)).astype(np.float32)
        self.states = rng.standard_normal((B, O)).astype(np.float32)
        self.actions = rng.standard_normal((B, A)).astype(np.float32)
        self.returns = rng.standard_normal(B).astype(np.float32)
        self.adv = (rng.standard_normal(B) * 2 + 0.3).astype(np.float32)
        pool = np.arange(B)
        self.kinks = []
        if self.act == nets.ACT_RELU:       # only rows without a unit at its kink, in either network, any layer
            self.kinks = kink_entries(ps, _f64(self.pp), self.states, KINK) + kink_entries(cs, _f64(self.cp), self.states, KINK)
            pool = np.setdiff1d(pool, np.array([k[1] for k in self.kinks], dtype=np.int64))
        self.pool = pool
        self.idx = pool[rng.permutation(pool.size)[:mb]].astype(np.int32)
        mean, _ = nets.forward(ps, self.pp, self.states)
        self.logp = (oppo.gaussian_log_prob(self.actions, mean, self.pp[ps.logstd:ps.logstd + A][None, :])
                     + 0.05 * rng.standard_normal(B)).astype(np.float32)
        self._built = True
        return self

    def batch(self, dtype):
        c, i = self.build(), self.build().idx
        t = lambda a: a.astype(dtype)
        return t(c.states[i]), t(c.actions[i]), t(c.logp[i]), t(c.returns[i]), oppo.normalize_advantages(t(c.adv[i]))

    def evaluate(self, dtype):
        c = self.build()
        return oppo.ppo_loss_and_grads(c.ps, c.pp.astype(dtype), c.cs, c.cp.astype(dtype), *self.batch(dtype), dtype(CLIP), dtype(ENT), dtype(CC))

    @functools.cached_property
    def oracle(self):
        """(loss, metrics, policy gradient, critic gradient) in float64: computed once per case"""
        return self.evaluate(np.float64)

    # ---- the whole update (section 5 of the issue): the pool as a rollout of T = 2 steps of N = mb environments
    @functools.cached_property
    def max_grad_norm(self):
        """half of the smaller gradient norm of the minibatch pass: clipping acts on both networks from the first update on"""
        _, _, gp, gc = self.oracle
        return float(np.float32(0.5 * min(np.linalg.norm(gp), np.linalg.norm(gc))))

    def update(self, dtype, key):
        """oppo.update from `key` in `dtype` -> (per-update metrics, new key, policy parameters, critic parameters, update count)"""
        c = self.build()
        mb, t = c.mb, lambda a: a.astype(dtype)
        pst, cst = oppo.TrainState(c.ps, t(c.pp)), oppo.TrainState(c.cs, t(c.cp))
        cfg = dict(minibatch_size=mb, nr_epochs=UPD_EPOCHS, learning_rate=LR, clip_range=dtype(CLIP), entropy_coef=dtype(ENT),
                   critic_coef=dtype(CC), max_grad_norm=self.max_grad_norm)
        out, new_key, _ = oppo.update(pst, cst, t(c.states).reshape(2, mb, c.O), t(c.actions).reshape(2, mb, c.A), t(c.adv).reshape(2, mb),
                                      t(c.returns).reshape(2, mb), None, t(c.logp).reshape(2, mb), key, cfg)
        return out, new_key, pst.params, cst.params, pst.count

    @functools.cached_property
    def update64(self):
        from oracle import prng
        return self.update(np.float64, prng.prng_key(5))


def fp16_window(c):
    """the largest operands the split engine turns into fp16 planes, from the float64 oracle: |weight| of the hidden layers, |activation|
    of every layer, and the per-sample gradient dZ of every layer times bx_grad_scale(mb)"""
    c.build()
    s, a, lp, r, madv = c.batch(np.float64)
    out = dict(weight=0.0, act=float(np.abs(s).max()), grad_scaled=0.0)
    for spec, par, policy in ((c.ps, _f64(c.pp), True), (c.cs, _f64(c.cp), False)):
        y, cache = nets.forward(spec, par, s)
        for L in spec.layers:
            out["weight"] = max(out["weight"], float(np.abs(par[L["W"]:L["W"] + L["in"] * L["out"]]).max()))
        out["act"] = max([out["act"]] + [float(np.abs(h).max()) for h in cache["h"]])
        if policy:                              # the loss seeds of ppo_loss_and_grads
            logstd = par[spec.logstd:spec.logstd + c.A][None, :]
            zs = (a - y) / np.exp(logstd)
            ratio = np.exp((-0.5 * zs ** 2 - 0.5 * oppo.LOG_2PI - logstd).sum(axis=1) - lp)
            inside = (ratio >= 1 - CLIP) & (ratio <= 1 + CLIP)
            d_out = (np.where(inside | (-madv * ratio > -madv * np.clip(ratio, 1 - CLIP, 1 + CLIP)), -madv, 0) * ratio / c.mb)[:, None] * (zs / np.exp(logstd))
        else:
            d_out = (CC / c.mb) * (y.reshape(-1) - r)[:, None]
        H = spec.head
        dh = d_out @ par[H["W"]:H["W"] + H["in"] * H["out"]].reshape(H["in"], H["out"]).T
        for li in range(len(spec.layers) - 1, 0, -1):       # (the first layer's dZ is consumed in fp32 registers)
            L = spec.layers[li]
            dz = dh * nets._act_grad_from_out(cache["h"][li], spec.act)
            out["grad_scaled"] = max(out["grad_scaled"], float(np.abs(dz).max()) * npth.bx_grad_scale(c.mb))
            dh = dz @ par[L["W"]:L["W"] + L["in"] * L["out"]].reshape(L["in"], L["out"]).T
        out["grad_scaled"] = max(out["grad_scaled"], float(np.abs(dh).max()) * npth.bx_grad_scale(c.mb))
    return out


def compare(c, met, gp, gc):
    """device metrics [>= 5] and flat gradients against the case's float64 oracle -> ({name: (got, expected, allowed)} for the metrics,
    {network[.block]: ||dg|| / ||g||}); nothing is asserted here"""
    loss_e, met_e, gp_e, gc_e = c.oracle
    m = _f64(met)
    rows = {name: (m[i], float(met_e[name]), atol + rtol * abs(float(met_e[name]))) for i, (name, rtol, atol) in enumerate(METRICS)}
    rows["policy_ratio/clip_fraction"] = (m[4], float(met_e["policy_ratio/clip_fraction"]), 1.5 / c.mb)
    rows["loss"] = (m[0] - ENT * m[2] + CC * m[1], float(loss_e), 1e-6 + 1e-5 * abs(float(loss_e)))
    report = {}
    for name, got, exp, spec in (("policy", gp, gp_e, c.ps), ("critic", gc, gc_e, c.cs)):
        report[name] = rel(got, exp)
        for bname, off, ln in blocks(spec):
            report[f"{name}.{bname}"] = rel(got[off:off + ln], exp[off:off + ln])
    return rows, report


_E, _T, _R = nets.ACT_ELU, nets.ACT_TANH, nets.ACT_RELU
# name, O, hidden, A, mb [, act, ln]: the issue's table (what each reaches: tests/test_ppo_cases.py's branch list), and below it the
# cases added for branches none of those reaches
_TABLE = [
    Case("narrow", 1, (512, 256, 128), 1, 4096),
    Case("edge32", 32, (512, 256, 128), 8, 4128),
    Case("h2_512", 31, (512, 512, 128), 8, 4160),
    Case("h2_384", 17, (512, 384, 128), 3, 4096, seed=103),      # (seed 3: the float32 evaluation's 3-entry logstd block at 5.6e-6, over half the bar)
    Case("h2_128", 17, (512, 128, 128), 6, 4096),
    Case("k64_ragged", 17, (512, 256, 64), 6, 5001),
    Case("k256", 17, (512, 256, 256), 6, 4096),
    Case("k100", 17, (512, 256, 100), 6, 4096),
    Case("two_layer", 17, (512, 256), 6, 4096),
    Case("act9", 17, (512, 256, 128), 9, 4096),
    Case("mid", 17, (512, 256, 128), 6, 8256, defaults=True),
    Case("wide376", 376, (512, 256, 128), 17, 4096),
    Case("wide33", 33, (512, 256, 128), 6, 4096),
    Case("flax256", 17, (256, 256), 6, 4096, _T, False),
    Case("flax64", 24, (64, 64), 4, 4100, _T, False),
    Case("flax512w", 40, (512, 512), 6, 4096, _T, False),
    Case("flax192", 17, (192, 192), 6, 4096, _T, False),
    Case("tail_tanh", 17, (256, 256, 128), 6, 4096, _T, False),
    Case("tail_relu", 17, (256, 128, 128), 6, 4096, _R, False),
    # hidden[1] = 64 is no multiple of 128: the fused first-layer backward without its split images (k_frag_reorder + the exact-fp32
    # k_dx_l1bwd), and a twin pass that twin_shapes_ok admits but twin_images turns down
    Case("h2_64", 17, (512, 64, 128), 6, 4096),
    # one hidden layer: the head kernel's dZ is the first layer's, no hidden GEMM at all
    Case("one_layer", 17, (256,), 6, 4096, _T, False),
    # ... and with LayerNorm: k_l1fwd_mfma forward, LayerNorm' alone left to the first-layer backward, the generic head at K = 512
    Case("one_layer_ln", 17, (512,), 6, 4096),
    # the `hidden[1] <= 512` terms of tail_shape_ok and l1fused_supported (mlp_check_desc accepts any multiple of 4 above the first
    # layer): no tail, and the 512-ELU-LayerNorm first layer's backward unfused (k_gemm_dx + k_l1<bwd> + the skinny weight gradient)
    Case("h2_640", 17, (512, 640, 128), 6, 4096),
    # Ant's 105 observations and 8 actions: a padded stride of 108, row records of 128 floats in the whole-update entries
    # (seed 23: two policy entries of the float32 numpy trajectory leave 2e-5 + 1e-3 |e|, at 6e-5: Adam on a gradient that is rounding noise)
    Case("wide105", 105, (512, 256, 128), 8, 4096, seed=123),
]
for _i, _c in enumerate(_TABLE):
    _c.seed = _i if _c.seed is None else _c.seed
CASES = {c.name: c for c in _TABLE}
NAMES = tuple(CASES)
RUNS = [(c.name, label) for c in _TABLE for label, _, _ in c.settings()]

# shapes the pass refuses (net_paths.ppo_refusal gives code and message): name -> (O, hidden, A, act, ln, mb)
REFUSED = {
    "h0_96": (17, (96, 96), 6, _T, False, 4096),
    "hidden_130": (17, (512, 256, 130), 6, _E, True, 4096),
    "head_512x16": (17, (512, 512), 16, _T, False, 4096),
    "wide_ln_one_layer": (40, (512,), 6, _E, True, 4096),
}


def case(name):
    return CASES[name].build()
