"""Helpers shared by the PPO-DTRL shape tests (test_dtrl_cases.py, test_gpu_dtrl_shapes.py, test_gpu_dtrl_update_shapes.py): the case
table of one minibatch's loss (rlx_dtrl_loss_f32) and of the whole update (rlx_dtrl_update_f32) over what dtrl.hip's host checks accept
and tests/test_gpu_dtrl*.py do not run, and the inputs both entry points must refuse.

A LossCase holds the arguments of dtrl_twin.case and, computed once and shared by every test, its inputs, the float64 twin's result and
the float32 twin's.  Unless a case says otherwise: obs 7, hidden (64,), LayerNorm + ELU, "mixed" (every third row above the mean bound,
the others below it; covariance projection active), old log-probs built from the twin's log-prob of the current policy (logp="policy").

Bars (test_gpu_dtrl.py's): the 12 metrics 1e-5 of max(|value|, 1); policy (head and body) and critic gradient 1e-5 relative L2; eta and
d logstd as derived below.  The float32 twin must hold each within half (test_dtrl_cases.py)."""
import functools

import numpy as np

import dtrl_twin as tw
from oracle import nets, ppo, prng

BAR = 1e-5
# eta (relative) and d logstd (L2 relative to max(norm, entropy_coef)): the largest error of the float32 twin against the float64 twin
# over THIS table, measured on the CPU (test_dtrl_cases.py prints both and holds every case to half the bar), times 8 for reduction
# order.  The float32 twin finds the covariance root in double, as k_dtrl_cov_proj does (dtrl_twin.CovProj): bisecting a float32 KL
# left eta 1.7e-5 off at cov_1e4 on one CPU and 3.3e-4 on another, which is the bisection's noise and no property of the device.
#   eta     2.88e-7 at adv_1025 (next: 2.69e-7 adv_1025_ce, 2.44e-7 in_6)
#   dlogstd 2.44e-6 at w64i_19 (next: 2.23e-6 w64_2, 2.17e-6 rows2_4100)
ETA_F32_MAX, DLOGSTD_F32_MAX = 2.88e-7, 2.44e-6
ETA_TOL, DLOGSTD_TOL = 8 * ETA_F32_MAX, 8 * DLOGSTD_F32_MAX
I_ETA = tw.METRICS.index("projection/eta_cov")
I_CLIP = tw.METRICS.index("policy_ratio/clip_fraction")


def rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30))


def figures(c, got_met, got_gp, got_gc, met, gp, gc):
    """the five figures of test_gpu_dtrl.py of a result against the float64 twin's"""
    ls = c["pspec"].logstd
    got_met, got_gp = np.asarray(got_met, np.float64), np.asarray(got_gp, np.float64)
    return {"metrics": float(np.max(np.abs(got_met - met) / np.maximum(np.abs(met), 1.0))), "policy": rel(got_gp[:ls], gp[:ls]),
            "critic": rel(got_gc, gc), "eta": float(abs(got_met[I_ETA] - met[I_ETA]) / max(met[I_ETA], 1e-30)),
            "dlogstd": float(np.linalg.norm(got_gp[ls:] - gp[ls:]) / max(np.linalg.norm(gp[ls:]), c["h"]["entropy_coef"]))}


class LossCase:
    def __init__(self, name, A, mb, modes="mixed", cov_margin=2.0, **kw):
        """modes: "mixed" (mean projection on a third of the rows + covariance), "mixed_all" (+ entropy), "cov", "cov_ent", or a
        (mean, cov, entropy) triple"""
        self.name, self.A, self.mb, self.cov_margin = name, A, mb, cov_margin
        mixed = modes in ("mixed", "mixed_all")
        trip = {"mixed": (1, 1, 0), "mixed_all": (1, 1, 1), "cov": (0, 1, 0), "cov_ent": (0, 1, 1)}.get(modes, modes)
        self.mean_on, self.cov_on, self.ent_on, self.mixed = bool(trip[0]), bool(trip[1]), bool(trip[2]), mixed
        self.kw = dict(dict(hidden=(64,), logp="policy", mixed=mixed), **kw)
        self.seed = 0

    @functools.cached_property
    def c(self):
        return tw.case(20261126 + self.seed, self.A, self.mb, int(self.mean_on), int(self.cov_on), int(self.ent_on), **self.kw)

    @functools.cached_property
    def twin64(self):
        """(loss, metrics [12], policy gradient, critic gradient, info) in float64: computed once per case"""
        return tw.run_case(self.c)

    @functools.cached_property
    def twin32(self):
        import torch
        return tw.run_case(self.c, torch.float32)

    def margins_ok(self):
        return tw.margins_ok(self.c, self.twin64[4], self.cov_margin)


_WIDE = dict(obs=48, hidden=(512, 256, 128))
_NEG = dict(old_ls_mean=-2.5, step=0.37)
# A = 33 and 64.  With dtrl_twin.case's defaults (rollout logstd near 0, actions a rollout standard deviation from the rollout means,
# the policy's logstd 0.5 below) a row's log-prob is a sum of up to 64 terms near -1.8, about -110, which float32 knows to 7e-6: the
# float32 twin's policy gradient was 5.2e-6 .. 7.2e-6 off at w64i_2, w64_7 and rows2_4100, past half the bar of 1e-5.  That is the
# number format, not a kernel (the device forms this sum in double).  Rollout logstd near -0.75 and actions within 0.2 standard
# deviations keep the terms near 0 and the log-prob within +-4; the float32 twin is then at most 3.1e-6 off.
_MANY = dict(old_ls_mean=-0.75, act_scale=0.2)
_TABLE = [
    # ---- sub-group widths the 60 cases leave out: W = 2; W = 16 with every lane a component; W = 64 with idle lanes and full, where
    #      a workgroup holds exactly four rows (2 rows: half a workgroup; 5, 7: a second workgroup with 1 / 3 rows; 19: five workgroups)
    LossCase("w2_33", 2, 33), LossCase("w2_257", 2, 2 * 128 + 1),
    LossCase("w16_5", 16, 5), LossCase("w16_67", 16, 4 * 16 + 3), LossCase("w16_all_67", 16, 4 * 16 + 3, "mixed_all"),
    LossCase("w64i_2", 33, 2, **_MANY), LossCase("w64i_5", 33, 5, **_MANY), LossCase("w64i_19", 33, 4 * 4 + 3, **_MANY),
    LossCase("w64_2", 64, 2, **_MANY), LossCase("w64_7", 64, 7, **_MANY), LossCase("w64_cov_7", 64, 7, "cov", **_MANY),
    # ---- the row loop's second pass: DT_MAX_BLOCKS workgroups of four rows cover 4096, rows 4096..4099 are the second trip of the
    #      first workgroup alone (its four waves make it, every other wave of the grid does not)
    LossCase("rows2_4100", 64, 4100, **_MANY),
    # ---- k_dtrl_adv_stats' second trip (thread 0 alone; threads 0..75) and k_dtrl_finish over 33 / 35 slabs
    LossCase("adv_1025_ce", 5, 1025, "cov_ent"), LossCase("adv_1100_ce", 5, 1100, "cov_ent"),
    LossCase("adv_1025", 5, 1025), LossCase("adv_1100", 5, 1100),
    # ---- networks: the reference's default; the widest LayerNorm layers (k_ln_act_wide's ELU branch past D = 64); no LayerNorm
    LossCase("ref_default", 12, 9, **_WIDE),
    LossCase("ln_elu_768", 3, 5, hidden=(768, 64)),
    LossCase("ln_tanh_512", 3, 5, hidden=(512,), act=nets.ACT_TANH),
    LossCase("noln_1024", 3, 5, hidden=(1024, 64), ln_first=False),
    LossCase("tanh_noln_2h", 8, 9, hidden=(128, 192), act=nets.ACT_TANH, ln_first=False),
    # ---- in_dim no multiple of four: k_dtrl_gather pads 3, 3 and 2 columns
    LossCase("in_1", 3, 9, obs=1), LossCase("in_5", 3, 9, obs=5), LossCase("in_6", 3, 9, obs=6),
    # ---- hp->critic_states: wider, narrower, and as wide as the policy's observations with other contents
    LossCase("cs_wide", 3, 9, obs=5, cobs=11, chidden=(128, 64)),
    LossCase("cs_narrow", 17, 40, obs=9, cobs=4), LossCase("cs_same", 17, 40, obs=7, cobs=7),
    # ---- the covariance step: a bound 10^4 below kl_cov (14 doublings, eta 1.6e4) and one a factor 2 below (one doubling; the
    #      branch margin of this case is 1.5, which the double-precision kl_cov of the device cannot be near)
    LossCase("cov_1e4", 8, 9, "cov", cov_ratio=1e4), LossCase("cov_2", 8, 9, "cov", cov_ratio=2.0, cov_margin=1.5),
    # ---- rollout logstd near -2.5: H(so) and beta negative, a fractional global_step / total_timesteps.  Entropy projection on
    #      (policy logstd 0.5 below the rollout's) and off (2.0 above it: the projected entropy stays above beta)
    LossCase("negH_3_on", 3, 9, "mixed_all", ls_offset=-0.5, **_NEG), LossCase("negH_8_on", 8, 9, "mixed_all", ls_offset=-0.5, **_NEG),
    LossCase("negH_3_off", 3, 9, ls_offset=2.0, **_NEG), LossCase("negH_8_off", 8, 9, ls_offset=2.0, **_NEG),
]
for _i, _c in enumerate(_TABLE):
    _c.seed = 100 * _i
CASES = {c.name: c for c in _TABLE}
NAMES = tuple(CASES)
REPEAT_NAMES = ("rows2_4100", "ref_default", "cs_wide")


# ---- the whole update
class UpdateCase:
    """rlx_dtrl_update_f32 as test_gpu_dtrl_update.py runs it (|logstd| small, cov_bound 1e-6 reached from the second step on, the
    entropy projection off) at another schedule: E epochs of M minibatches of mb rows from opt_count0 earlier steps, whose moments and
    parameters are those of a twin run of opt_count0 steps"""

    def __init__(self, name, A=3, E=2, M=2, mb=9, opt_count0=0, given=True, cobs=None, scheme=1, clip=False, poison=None, seed=0):
        self.name, self.A, self.E, self.M, self.mb, self.opt_count0, self.given = name, A, E, M, mb, opt_count0, given
        self.cobs, self.scheme, self.clip, self.poison, self.seed = cobs, scheme, clip, poison, seed
        self.B, self.n_upd = M * mb, E * M

    @functools.cached_property
    def built(self):
        """-> dict: c (inputs), key, idx [n_upd, mb], lrs, start (p, pm, pv, q, cm, cv as float32 arrays), twin (metrics [n_upd, 14],
        infos, policy TrainState, critic TrainState after the update)"""
        A, B, f32 = self.A, self.B, lambda v: np.asarray(v, np.float32).astype(np.float64)
        c = tw.case(20271126 + self.seed, A, self.mb, 1, 1, 0, B=B, hidden=(64,), cobs=self.cobs)
        h, ls = c["h"], c["pspec"].logstd
        c["pp"][ls:] = f32(np.random.default_rng(self.seed).uniform(-0.04, 0.04, A))
        c["old_logstd"], c["global_step"], h["cov_bound"] = c["pp"][ls:].copy(), 1000.0, 1e-6
        # the rows' maha starts near 0.01 and moves with every step of the policy: a bound of 2.5e-4 keeps every row of every step
        # a factor 4 above it (with the rollout means computed, maha is 0 at the first step and past 2 x 1.25e-3 from the second)
        h["mean_bound"] = 2.5e-4 if self.given else 1.25e-3
        ps, cs = ppo.TrainState(c["pspec"], c["pp"]), ppo.TrainState(c["cspec"], c["cp"])
        if self.opt_count0:     # earlier steps on rows of their own kind: the moments and the count a later iteration starts from
            w = tw.case(20281126 + self.seed, A, self.mb, 1, 1, 0, B=B, hidden=(64,), cobs=self.cobs)
            w["logp_old"] = f32(tw.run_case(dict(w, pp=c["pp"], cp=c["cp"], old_logstd=c["old_logstd"]))[4]["logp"])
            idx0 = np.arange(self.opt_count0 * self.mb).reshape(self.opt_count0, self.mb) % B
            tw.update(ps, cs, w["states"], w["actions"], w["old_means"], c["old_logstd"], w["logp_old"], w["returns"], w["adv"], idx0,
                      np.full(self.opt_count0, 1e-3), 1000.0, dict(h, cov_bound=1e3), cstates=w["cstates"])
            for st in (ps, cs):     # the device holds float32 state
                st.params, st.m, st.v = f32(st.params), f32(st.m), f32(st.v)
            c["pp"], c["cp"] = ps.params.copy(), cs.params.copy()
            c["old_logstd"] = c["pp"][ls:].copy()
        if not self.given:      # the rollout's means ARE the incoming policy's (test_gpu_dtrl_update.py)
            c["old_means"] = f32(nets.forward(c["pspec"], c["pp"], c["states"])[0])
        c["logp_old"] = f32(tw.run_case(c)[4]["logp"] + np.random.default_rng(3 + self.seed).uniform(-0.02, 0.02, B))
        if self.poison == "returns":
            c["returns"][0] = np.nan
        if self.poison == "advantages":
            c["adv"][0] = np.inf
        key = prng.prng_key(5 + self.seed)
        key_out, idx = prng.ppo_minibatch_indices(key, B, self.E, self.M, self.mb, bool(self.scheme))
        idx = np.asarray(idx).reshape(self.n_upd, self.mb)
        lrs = np.linspace(3e-3, 5e-4, self.n_upd).astype(np.float32)
        start = tuple(np.asarray(v, np.float32) for v in (ps.params, ps.m, ps.v, cs.params, cs.m, cs.v))
        if self.clip:           # both networks clipped at every step: half the smallest norm of an unclipped twin run
            import copy
            met0, _ = tw.update(copy.deepcopy(ps), copy.deepcopy(cs), c["states"], c["actions"], c["old_means"], c["old_logstd"],
                                c["logp_old"], c["returns"], c["adv"], idx, lrs.astype(np.float64), 1000.0, dict(h, max_grad_norm=1e9),
                                cstates=c["cstates"])
            h["max_grad_norm"] = float(np.float32(0.5 * met0[:, 12:14].min()))
        met, infos = tw.update(ps, cs, c["states"], c["actions"], c["old_means"], c["old_logstd"], c["logp_old"], c["returns"], c["adv"], idx,
                               lrs.astype(np.float64), 1000.0, h, cstates=c["cstates"])
        return dict(c=c, key=key, key_out=np.asarray(key_out, np.uint32), idx=idx, lrs=lrs, start=start, twin=(met, infos, ps, cs))


UPDATES = {u.name: u for u in (
    UpdateCase("e1_m1", E=1, M=1, seed=1),
    UpdateCase("e2_m3_count3", E=2, M=3, opt_count0=3, seed=2),
    UpdateCase("a16_cstates_null_means", A=16, cobs=5, given=False, seed=3),
    UpdateCase("both_clipped", clip=True, seed=4),
    UpdateCase("other_scheme", scheme=0, seed=5),
    UpdateCase("prefetch", seed=6),
    UpdateCase("skip_critic", E=1, M=1, poison="returns", seed=7),
    UpdateCase("skip_policy", E=1, M=1, poison="advantages", seed=8),
)}
# the twin's cov_on per step: kl_cov is 0 at the first step of an iteration and past the bound of 1e-6 from the second on
UPDATE_COV_ON = lambda u: [i > 0 for i in range(u.n_upd)]

# ---- refusals.  name -> (what to change, the error class, what the message must name).  "p." / "c.": a field of the policy's / the
# critic's rlx_mlp_desc (hidden: the whole list); "h.": a DtrlHparams field; "mb": the minibatch rows; "cobs": the critic's in_dim
# with hp->critic_states NULL
EINVAL, EUNSUP = -1, -4          # RLX_EINVAL, RLX_EUNSUP (include/rlx_hip.h)
_WIDTH = "hidden"
REFUSED = {
    "n_hidden_0": ({"p.hidden": ()}, EUNSUP, "hidden layers"), "n_hidden_4": ({"c.hidden": (64, 64, 64, 64)}, EUNSUP, "hidden layers"),
    "act_relu": ({"p.act": nets.ACT_RELU}, EUNSUP, "act"),
    "width_32": ({"p.hidden": (32,)}, EUNSUP, _WIDTH), "width_96": ({"c.hidden": (64, 96)}, EUNSUP, _WIDTH),
    "width_1088": ({"p.hidden": (64, 1088)}, EUNSUP, _WIDTH),
    "ln_elu_832": ({"p.hidden": (832,)}, EUNSUP, _WIDTH), "ln_tanh_576": ({"c.hidden": (576,), "p.act": nets.ACT_TANH, "c.act": nets.ACT_TANH}, EUNSUP, _WIDTH),
    "policy_no_logstd": ({"p.has_logstd": 0}, EUNSUP, "has_logstd"), "critic_logstd": ({"c.has_logstd": 1}, EUNSUP, "has_logstd"),
    "act_dim_0": ({"p.out_dim": 0}, EUNSUP, "out_dim"), "act_dim_65": ({"p.out_dim": 65}, EUNSUP, "out_dim"),
    "critic_out_2": ({"c.out_dim": 2}, EUNSUP, "out_dim"), "in_dim_0": ({"p.in_dim": 0, "c.in_dim": 0}, EINVAL, "in_dim"),
    "mean_bound_0": ({"h.mean_bound": 0.0}, EINVAL, "mean_bound"), "mean_bound_neg": ({"h.mean_bound": -0.01}, EINVAL, "mean_bound"),
    "cov_bound_0": ({"h.cov_bound": 0.0}, EINVAL, "cov_bound"), "cov_bound_neg": ({"h.cov_bound": -1e-3}, EINVAL, "cov_bound"),
    "total_timesteps_0": ({"h.total_timesteps": 0.0}, EINVAL, "total_timesteps"),
    "total_timesteps_neg": ({"h.total_timesteps": -1.0}, EINVAL, "total_timesteps"),
    "one_row": ({"mb": 1}, EUNSUP, "two rows"),
    "in_dims_differ": ({"c.in_dim": 9}, EINVAL, "critic_states"),
}
REFUSED_UPDATE = dict(REFUSED, **{
    "ragged_batch": ({"mb": 4}, EINVAL, "minibatch_size"), "epochs_0": ({"E": 0}, EINVAL, "nr_epochs"),
    "opt_count_neg": ({"opt_count": -1}, EINVAL, "opt_count_io"), "world_2": ({"world": 2}, EUNSUP, "world size"),
})
