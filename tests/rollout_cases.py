"""Helpers shared by the shape tests of the fused acting step (test_rollout_cases.py, test_gpu_rollout_shapes.py): a Python mirror
of rlx_ppo_rollout_step_supported and of the path choices k_rollout_step makes from a shape (rl-x_amd/csrc/rollout.hip), a named
case table, and a Case: seeded float32 parameters (nets.init_params + 0.05 N(0,1) on every entry, so that every bias, LayerNorm
scale / bias and logstd is non-trivial and differs per column), per-dimension asymmetric action bounds, the env oracle, and the
expected outputs of one step from the float64 oracle.

Bars (the ones tests/test_gpu_rollout.py holds this kernel to; rtol, atol against the float64 oracle on IDENTICAL float32 inputs):
  value                     1e-5, 1e-5   one float32 forward pass of the critic
  action, processed action  3e-5, 1e-5   mean + std * eps: the N(0,1) draw is erfinv of a float32 uniform, ill-conditioned in the
                                         tails (two float32 evaluations of the same polynomial differ by ~1.6e-5 relative at
                                         |eps| ~ 4); the uniform bits are compared exactly in test_gpu_prng.py.  The processed
                                         action is an affine map of the clipped action with |slope| (hi - lo) / 2 <= 3.5
  log-prob                  3e-5, 2e-5   a sum over A terms -0.5 ((a - mu) / sd)^2 - 0.5 log 2 pi - logstd
  reward                    1e-5, 1e-5   float32 on both sides, the env driven by the device's own processed action
  final_obs, next obs       2e-5, 2e-6   Box-Muller tails: the device's log / cos against libm
Exact: terminated, ep_step, the returned key (prng.split), episode_stats[0] (finished episodes).
test_rollout_cases.py holds a plain float32 numpy evaluation of every case to half of each of the first three bars, so that a
miss on the device is the kernel's and not the inputs'.  Measured there (largest fraction of a bar per case, float32 numpy against
float64): one512_a32 0.20, one320_fit 0.02, one320_over 0.03, min 0.002, valu_ln_relu 0.11, mfma_noln 0.11, mfma_two 0.07,
three_valu 0.17 (0.25 with the legacy key scheme's draws), mixed 0.19."""
import numpy as np

from oracle import env as oenv, nets, ppo as oppo, prng
from rlx_amd.hip import mlp_desc

BARS = dict(value=(1e-5, 1e-5), action=(3e-5, 1e-5), processed=(3e-5, 1e-5), logp=(3e-5, 2e-5), reward=(1e-5, 1e-5),
            obs=(2e-5, 2e-6))

# ------------------------------------------------------------------------------------------- mirror of rollout.hip's constants
RO_ROWS, RO_MAXH, RO_MAXN, G_BK = 32, 512, 256, 32
RO_A1 = RO_ROWS * (RO_MAXN + 1)          # activation buffer 1 (floats)
RO_BS = G_BK * (RO_MAXN + 4)             # weight stage
MAX_IN, MAX_OUT = 32, 1024 // RO_ROWS


def net_supported(in_dim, hidden, out_dim):
    """fill_net"""
    n = len(hidden)
    if n < 1 or n > 3 or in_dim < 1 or in_dim > MAX_IN or out_dim < 1:
        return False
    if hidden[0] < 64 or hidden[0] % 64 != 0 or hidden[0] > RO_MAXH:
        return False
    for l in range(1, n):
        if hidden[l] not in (128, 256) or hidden[l - 1] % (2 * G_BK) != 0:
            return False
    return out_dim * RO_ROWS <= 1024


def step_supported(p_in, p_hidden, p_out, p_logstd, c_in, c_hidden, c_out):
    """rlx_ppo_rollout_step_supported"""
    return bool(net_supported(p_in, p_hidden, p_out) and net_supported(c_in, c_hidden, c_out) and p_in == c_in and p_logstd
                and c_out == 1)


def layer0_path(in_dim, hidden):
    """k_rollout_step's first-layer branch: the matrix pipe takes hidden[0] == 512, the VALU everything else"""
    return "mfma" if hidden[0] == 512 and in_dim <= 32 else "valu"


def head_floats(hidden, out_dim):
    return hidden[-1] * out_dim


def head_stage_floats(hidden):
    """LDS floats the head's weights are staged into: behind one hidden layer A1 | Bs (both free), else the weight stage"""
    return RO_A1 + RO_BS if len(hidden) == 1 else RO_BS


def fp32_layer_trips(K):
    """fused_layer: trips of its two-tile K loop"""
    return K // (2 * G_BK)


def bx_main_loop(K):
    """fused_layer_bx: whether its four-block main loop runs at all (`g + 4 < K / 16`); at K = 64 only the peeled tail does"""
    return 4 < K // 16


# ------------------------------------------------------------------------------------------------------------------ the cases
NOISE_ROW_OFFSET, EXTRA_ROWS = 128, 131          # n_global = N + 131
ENV = dict(seed=11, horizon=3, p_term=0.1, reward_noise=0.1, env_id_offset=37)    # horizon 3: every env finishes within 3 steps
STEPS = 3

TANH, ELU, RELU = nets.ACT_TANH, nets.ACT_ELU, nets.ACT_RELU
#        name           seed  O   A   N   policy (hidden, act, LN)        critic (None: the policy's)        clip  schemes
TABLE = {
    "one512_a32":   (301, 32, 32, 70, ((512,), ELU, True), None, True, (1,)),
    "one320_fit":   (302, 7, 26, 33, ((320,), TANH, False), None, False, (1,)),
    "one320_over":  (303, 7, 27, 33, ((320,), TANH, False), None, False, (1,)),
    "min":          (304, 1, 1, 1, ((64, 128), TANH, False), None, False, (1,)),
    "valu_ln_relu": (305, 31, 17, 33, ((448, 256), RELU, True), None, True, (1,)),
    "mfma_noln":    (306, 32, 32, 70, ((512, 256, 128), ELU, False), None, False, (1,)),
    "mfma_two":     (307, 2, 3, 32, ((512, 128), TANH, True), None, False, (1,)),
    "three_valu":   (308, 5, 9, 70, ((192, 128, 256), ELU, True), None, True, (1, 0)),
    "mixed":        (309, 17, 6, 70, ((256, 256), TANH, False), ((512, 256, 128), ELU, True), True, (1,)),
}
NAMES = list(TABLE)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class ClampedColsEnv(oenv.RandomObsEnvOracle):
    """the fault `obs[min(j, O - 1)]` in place of `obs[j % O]` (test_rollout_cases.py)"""

    def target_cols(self):
        return np.minimum(np.arange(self.A), self.O - 1)


class Case:
    def __init__(self, name):
        seed, O, A, N, pol, cri, clip, schemes = TABLE[name]
        cri = cri or pol
        self.name, self.O, self.A, self.N, self.clip, self.schemes = name, O, A, N, clip, schemes
        rng = np.random.default_rng(seed)
        self.ps = nets.MLPSpec(O, pol[0], A, pol[1], pol[2], True)
        self.cs = nets.MLPSpec(O, cri[0], 1, cri[1], cri[2], False)
        self.pp = _f32(nets.init_params(self.ps, rng, 0.01) + 0.05 * rng.standard_normal(self.ps.n_params))
        self.cp = _f32(nets.init_params(self.cs, rng, 1.0) + 0.05 * rng.standard_normal(self.cs.n_params))
        self.pd = mlp_desc(O, self.ps.hidden, A, self.ps.act, self.ps.ln_first, True)
        self.cd = mlp_desc(O, self.cs.hidden, 1, self.cs.act, self.cs.ln_first, False)
        self.lo, self.hi = _f32(rng.uniform(-3.0, -0.5, A)), _f32(rng.uniform(0.5, 4.0, A))
        self.key = prng.prng_key(seed)
        self.n_global = N + EXTRA_ROWS
        self.has_images = len(self.ps.hidden) > 1 or len(self.cs.hidden) > 1      # one-layer nets have no layer for an image

    def supported(self):
        return step_supported(self.O, self.ps.hidden, self.A, True, self.O, self.cs.hidden, 1)

    def env(self, cls=oenv.RandomObsEnvOracle):
        e = cls(ENV["seed"], self.N, self.O, self.A, ENV["horizon"], ENV["p_term"], ENV["reward_noise"], ENV["env_id_offset"])
        e.reset()
        return e

    def variants(self):
        """(images, scheme) of every run of this case"""
        return [(im, s) for s in self.schemes for im in ((False, True) if self.has_images else (False,))]

    def noise(self, key, scheme):
        """-> (key after the step, this process's rows of the step's N(0,1) draws, float32)"""
        ks = prng.split(key, 2, bool(scheme))
        eps = prng.normal(ks[1], (self.n_global, self.A), bool(scheme))[NOISE_ROW_OFFSET:NOISE_ROW_OFFSET + self.N]
        return ks[0], eps

    def expected(self, obs, eps, dtype=np.float64, pp=None, cp=None, lo=None, hi=None, trace=None):
        """the oracle's step on float32 inputs, evaluated in `dtype` -> dict(action, value, logp, processed).  pp / cp / lo / hi:
        stand-ins for the case's own (the faults of test_rollout_cases.py); trace: a list that receives max |hidden activation|"""
        pp, cp = (self.pp if pp is None else pp).astype(dtype), (self.cp if cp is None else cp).astype(dtype)
        lo, hi = (self.lo if lo is None else lo).astype(dtype), (self.hi if hi is None else hi).astype(dtype)
        a, v, lp = oppo.get_action_and_value(self.ps, pp, self.cs, cp, obs.astype(dtype), eps.astype(dtype))
        if trace is not None:
            for spec, par in ((self.ps, pp), (self.cs, cp)):
                trace.append(max(float(np.abs(h).max()) for h in nets.forward(spec, par, obs.astype(dtype))[1]["h"]))
        return dict(action=a, value=v, logp=lp, processed=oppo.processed_action(a, self.clip, lo, hi))


def bar_fraction(name, got, exp):
    """max |got - exp| / (atol + rtol |exp|): 1 is the bar"""
    rtol, atol = BARS[name]
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return float(np.max(np.abs(got - exp) / (atol + rtol * np.abs(exp))))


def worst_fraction(got, exp, names=("action", "value", "logp", "processed")):
    return max(bar_fraction(k, got[k], exp[k]) for k in names)
