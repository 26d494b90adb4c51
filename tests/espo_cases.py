"""Shared by the ESPO tests: the reference fixture's cases (tests/golden/espo_reference.npz) and seeded random cases for the shape
envelope, each as what the twin (tests/espo_twin.py) and the library take."""
import os

import numpy as np

import espo_twin as tw

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "espo_reference.npz")
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = np.load(FIXTURE)
    return _Z


def n_cases():
    return int(fixture()["n_cases"])


class Case:
    """One problem: shapes, hyper-parameters, the flat rollout (float32-representable float64), indices, initial parameters."""

    def indices(self):
        """(pidx, cidx) for the twin: None when the nets read all columns"""
        return (None, None) if self.full_obs else (self.pidx, self.cidx)

    def state(self):
        return tw.new_state(self.p0, self.c0)

    def twin(self, st=None, max_epochs=None, **hp):
        """the twin's update from `st` (default: the initial state) -> (state, metrics, epochs_run, info)"""
        st = self.state() if st is None else st
        h = dict(self.h, **hp)
        pidx, cidx = self.indices()
        idx = self.idx if max_epochs is None else self.idx[:max_epochs]
        met, run, info = tw.update(st, self.LP, self.LC, self.states, self.actions, self.log_probs, self.advantages, self.returns, idx, h,
                                   pidx=pidx, cidx=cidx)
        return st, met, run, info


def load(c):
    z, k = fixture(), "c%d_" % c
    fc = Case()
    fc.z, fc.k = z, k
    fc.O, fc.A, fc.H, fc.T, fc.N, fc.mb, fc.E = (int(z[k + n]) for n in ("obs_dim", "act_dim", "hidden", "T", "N", "mb", "max_epochs"))
    fc.B = fc.T * fc.N
    fc.pidx, fc.cidx = z[k + "pidx"], z[k + "cidx"]
    fc.full_obs = len(fc.pidx) == fc.O and len(fc.cidx) == fc.O
    fc.h = dict(tw.HP)
    for n in ("max_ratio_delta", "entropy_coef", "critic_coef", "max_grad_norm", "learning_rate", "gamma", "gae_lambda"):
        fc.h[n] = float(z[k + n])
    fc.h["delta_calc_operator"] = str(z[k + "delta_calc_operator"])
    fc.LP, fc.LC = tw.layout(len(fc.pidx), fc.H, fc.A, True), tw.layout(len(fc.cidx), fc.H, 1, False)
    fc.p0, fc.c0 = tw.make_params(int(z[k + "param_seed"]), len(fc.pidx), len(fc.cidx), fc.A, fc.H)
    fc.states = z[k + "states"].reshape(fc.B, fc.O)
    fc.actions, fc.log_probs, fc.advantages, fc.returns = (z[k + n] for n in ("actions", "log_probs", "advantages", "returns"))
    fc.idx = z[k + "idx"]
    fc.low, fc.high = z[k + "low"].astype(np.float64), z[k + "high"].astype(np.float64)
    fc.metrics, fc.epochs_run, fc.stop_epoch = z[k + "metrics"], int(z[k + "epochs_run"]), int(z[k + "stop_epoch"])
    fc.sampled = lambda name: (z[k + name + "_idx"], z[k + name + "_val"], float(z[k + name + "_norm"]))
    return fc


def random_case(seed, O, A, H, B, mb, E, op="mean", Op=None, Oc=None, lr=2e-3, **hp):
    """A seeded problem of any shape: rollout rows around the policy's own actions, old log-probs 0.05 N off the policy's."""
    rng = np.random.default_rng(seed)
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    fc = Case()
    fc.O, fc.A, fc.H, fc.B, fc.mb, fc.E = O, A, H, B, mb, E
    fc.full_obs = Op is None and Oc is None
    fc.pidx = np.arange(O) if Op is None else np.sort(rng.choice(O, Op, replace=False))
    fc.cidx = np.arange(O) if Oc is None else np.sort(rng.choice(O, Oc, replace=False))
    fc.h = dict(tw.HP, delta_calc_operator=op, learning_rate=lr, **hp)
    fc.LP, fc.LC = tw.layout(len(fc.pidx), H, A, True), tw.layout(len(fc.cidx), H, 1, False)
    fc.p0, fc.c0 = tw.make_params(seed + 1, len(fc.pidx), len(fc.cidx), A, H)
    fc.states = f32(rng.standard_normal((B, O)))
    mean = tw.forward(fc.p0, fc.LP, fc.states[:, fc.pidx])[2]
    std = np.exp(fc.p0[fc.LP["logstd"][0]:])
    fc.actions = f32(mean + std * rng.standard_normal((B, A)))
    lp = tw.logprob_entropy(fc.p0, fc.LP, fc.states[:, fc.pidx], fc.actions)[0]
    fc.log_probs = f32(lp + 0.05 * rng.standard_normal(B))
    fc.advantages = f32(rng.standard_normal(B) * 1.5 + 0.3)
    fc.returns = f32(rng.standard_normal(B))
    fc.idx = tw.draw_indices(np.random.default_rng(seed + 2), B, mb, E)
    return fc


def margins_ok(info, rel=1e-3):
    """the generator's two conditions on a twin run: ratio_delta at least `rel` (relative) off the threshold at every epoch, and
    (median, even minibatch) the two middle values at least `rel` apart"""
    return bool(np.all(info["margin"] >= rel) and np.all(info["middle_gap"] >= rel))


# ------------------------------------------------------------------------------------------------- the library on a Case (GPU tests)
SENTINEL = -777.0
STATE_KEYS = ("p", "pm", "pv", "c", "cm", "cv")


def _rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


def f32_state(st):
    """a twin state rounded to what the device holds"""
    return {k: (v if k == "count" else np.asarray(v, np.float32).astype(np.float64)) for k, v in st.items()}


def espo_hp(h):
    from rlx_amd.hip import EspoHparams
    thr = h["max_ratio_delta"]
    return EspoHparams(float(thr) if np.isfinite(thr) else float("inf"), h["entropy_coef"], h["critic_coef"], h["max_grad_norm"], h["adam_b1"],
                       h["adam_b2"], h["adam_eps"], {"mean": 0, "median": 1}[h["delta_calc_operator"]])


def descs(fc):
    from rlx_amd.hip import ACT_TANH, mlp_desc
    return (mlp_desc(len(fc.pidx), [fc.H, fc.H], fc.A, ACT_TANH, False, True), mlp_desc(len(fc.cidx), [fc.H, fc.H], 1, ACT_TANH, False, False))


class Run:
    """one rlx_espo_update_f32 call on device copies of a twin state; metrics rows start as SENTINEL"""

    def __init__(self, ctx, dev, fc, st=None, max_epochs=None, chunk=None, two_streams=None, **hp):
        import torch
        t = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt))).to(dev)
        st = fc.state() if st is None else st
        h = dict(fc.h, **hp)
        idx = fc.idx if max_epochs is None else fc.idx[:max_epochs]
        nets = {k: t(st[k]) for k in STATE_KEYS}
        pd, cd = descs(fc)
        pidx, cidx = fc.indices()
        self.met = torch.full((idx.shape[0], 8), SENTINEL, device=dev)
        if chunk is not None:
            ctx.set_option("espo_chunk", chunk)
        if two_streams is not None:
            ctx.set_option("two_streams", two_streams)
        try:
            self.run, self.count = ctx.espo_update(
                pd, nets["p"], nets["pm"], nets["pv"], cd, nets["c"], nets["cm"], nets["cv"], t(fc.states), t(fc.actions), t(fc.log_probs),
                t(fc.returns), t(fc.advantages), t(idx, np.int32), st["count"], h["learning_rate"], espo_hp(h), self.met,
                pidx=None if pidx is None else t(pidx, np.int32), cidx=None if cidx is None else t(cidx, np.int32))
        finally:
            ctx.set_option("espo_chunk", 2)
            ctx.set_option("two_streams", 1)
        torch.cuda.synchronize()
        self.out = {k: v.cpu().numpy().astype(np.float64) for k, v in nets.items()}
        self.metrics = self.met.cpu().numpy().astype(np.float64)

    def same_bits(self, other, rows):
        return (all(self.out[k].tobytes() == other.out[k].tobytes() for k in STATE_KEYS) and
                self.metrics[:rows, :7].tobytes() == other.metrics[:rows, :7].tobytes() and self.run == other.run and self.count == other.count)


def check_against_twin(r, st0, st, met, run):
    """a Run against the twin's result from the state st0, at the project's bars: metrics 1e-5 of max(|value|, 1);
    vectors 1e-5 relative L2, second moments 5e-5, the parameter step 2e-4 where the gradient (the first moment) is not negligible;
    epochs_run exact; metrics rows past it untouched"""
    assert r.run == run and r.count == st["count"], (r.run, run)
    got = r.metrics[:run, :7]
    figures = {"metrics": float(np.max(np.abs(got - met) / np.maximum(np.abs(met), 1.0)))}
    sels = {}
    for key, mkey in (("p", "pm"), ("c", "cm")):
        m = st[mkey]
        sel = sels[key] = np.abs(m) > 1e-3 * np.sqrt(np.mean(m * m))
        p0 = np.asarray(st0[key], np.float32).astype(np.float64)
        figures.update({key: _rel(r.out[key], st[key]), mkey: _rel(r.out[mkey], st[mkey]), key + "v": _rel(r.out[key + "v"], st[key + "v"]),
                        key + "_step": _rel((r.out[key] - p0)[sel], (st[key] - p0)[sel])})
    print("espo figures:", {k: "%.2e" % v for k, v in figures.items()})
    bad = [(e, tw.METRICS[i], got[e, i], met[e, i]) for e in range(run) for i in range(7)
           if not abs(got[e, i] - met[e, i]) <= 1e-5 * max(abs(met[e, i]), 1.0)]
    assert not bad, bad
    assert np.all(r.metrics[run:] == SENTINEL) and np.all(r.metrics[:run, 7] == 0.0)
    for key in ("p", "c"):
        assert figures[key] < 1e-5 and figures[key + "m"] < 1e-5 and figures[key + "v"] < 5e-5, (key, figures)
        assert sels[key].mean() > 0.9, (key, sels[key].mean())
        assert figures[key + "_step"] < 2e-4, (key, figures)
