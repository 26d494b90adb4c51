"""What tools/tqc_bench.py, redq_bench.py, aqe_bench.py and droq_bench.py share: the shapes (obs 376, act 17, hidden 256), the
LeCun-normal networks, the seeded state and batches, the event timer, and the SAC updates the first three time beside their own.
The draws come from ONE generator in the order of the calls, so a tool's inputs are the same from run to run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rl-x_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

O, A, W = 376, 17, 256


def lecun(rng, in_dim, hidden, out_dim):
    parts, d = [], in_dim
    for h in list(hidden) + [out_dim]:
        parts += [(np.clip(rng.standard_normal((d, h)), -2, 2) * np.sqrt(1.0 / d) / 0.87962566103423978).ravel(), np.zeros(h)]
        d = h
    return np.concatenate(parts).astype(np.float32)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


class Bench:
    """one context, one generator, the policy's descriptor, and the args' --warmup / --iters"""

    def __init__(self, args):
        from rlx_amd.hip import ACT_RELU, Ctx, mlp_desc
        self.args = args
        self.dev = torch.device("cuda:0")
        self.ctx = Ctx(0)
        self.rng = np.random.default_rng(0)
        self.pd = mlp_desc(O, [W, W], 2 * A, ACT_RELU, False, False)

    def qdesc(self, out_dim=1):
        from rlx_amd.hip import ACT_RELU, mlp_desc
        return mlp_desc(O + A, [W, W], out_dim, ACT_RELU, False, False)

    def t(self, x):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(self.dev)

    def state(self, E, out_dim=1, relayout=None):
        """relayout: flat plain critic -> the flat critic of another layout (droq_bench.py's LayerNorm parameters)"""
        pp = lecun(self.rng, O, [W, W], 2 * A)
        pp[-(W * 2 * A + 2 * A):] *= 0.1                       # std ~ 1: the tanh rarely saturates
        P = self.t(pp)
        nets = [lecun(self.rng, O + A, [W, W], out_dim) for _ in range(E)]
        Q = self.t(np.concatenate([relayout(x) for x in nets] if relayout else nets))
        z = lambda: torch.zeros(1, device=self.dev)
        return dict(P=P, pm=torch.zeros_like(P), pv=torch.zeros_like(P), Q=Q, qm=torch.zeros_like(Q), qv=torch.zeros_like(Q), QT=Q.clone(),
                    la=z(), am=z(), av=z())

    def batch(self, G, B):
        rng, t = self.rng, self.t
        return (t(rng.standard_normal((G, B, O))), t(rng.standard_normal((G, B, O))), t(np.tanh(rng.standard_normal((G, B, A)))),
                t(rng.standard_normal((G, B))), t(rng.random((G, B)) < 0.1))

    def nets(self, qd, st):
        """the arguments every update call begins with"""
        return (self.pd, st["P"], st["pm"], st["pv"], qd, st["Q"], st["qm"], st["qv"], st["QT"], st["la"], st["am"], st["av"])

    def time_step(self, step, counters):
        """ms per call of step(key, *counters, metrics) -> (key, *counters), fed its own results"""
        from rlx_amd.hip import lib as L
        met = torch.zeros(10, device=self.dev)
        box = [L.prng_key(0)] + [0] * counters

        def fn():
            box[:] = step(*box, met)

        ms = timed(fn, self.args.warmup, self.args.iters)
        assert torch.isfinite(met).all(), met
        return ms

    def time_utd(self, update, qd, st, b, hp, row, **tail):
        """one high update-to-data update (two counters): prints `row`, its timing fields, then `tail`"""
        nets = self.nets(qd, st)
        ms = self.time_step(lambda key, q, pi, met: update(*nets, b, key, q, pi, hp, met), 2)
        G = int(hp.q_update_steps)
        print(json.dumps(dict(row, ms=round(ms, 3), calls_per_s=round(1000.0 / ms, 2), critic_steps_per_s=round(1000.0 * G / ms, 1), **tail)),
              flush=True)

    def run_sac(self, n, B):
        """n SAC updates (rlx_sac_update_f32, two scalar critics) per timed call"""
        from rlx_amd.hip import SacHparams
        st, b = self.state(2), tuple(x[0] for x in self.batch(1, B))
        hp = SacHparams(0.99, 0.005, -float(A), -20.0, 2.0, 3e-4, 3e-4, 3e-4, 0.9, 0.999, 1e-8)
        nets = self.nets(self.qdesc(), st)

        def step(key, count, met):
            for _ in range(n):
                key, count = self.ctx.sac_update(*nets, b, key, count, hp, met)
            return key, count

        ms = self.time_step(step, 1)
        print(json.dumps({"what": "%d_sac_updates" % n, "critics": 2, "batch": B, "ms": round(ms, 3), "ms_per_update": round(ms / n, 4)}),
              flush=True)
