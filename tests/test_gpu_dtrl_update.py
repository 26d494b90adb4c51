"""GPU: the whole PPO-DTRL update (rlx_dtrl_update_f32) with E = 2 epochs of M = 2 minibatches against the twin's loss + oracle/ppo.py's
float64 clip + Adam, with the rollout means given and with NULL (computed from the incoming policy).  Bars: tests/espo_cases.py's
(metrics 1e-5 of max(|value|, 1); vectors 1e-5 relative L2, second moments 5e-5, the parameter step 2e-4).
The policy's logstd is small in magnitude on purpose: kl_cov is a function of logstd - old logstd, and the device keeps logstd in
float32.  At logstd = -0.5 (one ulp 6e-8) a step of 3e-3 is known to 2e-5 of itself and eta with it -- measured there: kl_cov 1e-5
off, the policy gradient norm 1.6e-5 -- which is the storage format, not the kernels; at |logstd| < 0.05 an ulp is 4e-9."""
import numpy as np
import pytest
import torch

import dtrl_twin as tw
from oracle import nets, ppo
from rlx_amd.hip import lib as L
from test_gpu_dtrl import descs, hparams, rel

pytestmark = pytest.mark.gpu
E, M, MB, A = 2, 2, 9, 3
COV_BOUND = 1e-6


@pytest.mark.parametrize("given", [True, False])
def test_update_matches_the_twin(ctx, dev, given):
    B = M * MB
    c = tw.case(21, A, MB, 1, 1, 0, B=B)
    h = c["h"]
    # the call reads the rollout policy's logstd from the incoming parameters: kl_cov is 0 at the first step and grows past the bound
    # with the steps; the entropy bound has decayed to a thousandth of the entropy, so that projection stays the identity (behind
    # an active one a row whose ratio has left the clip range hands the covariance rule an exactly zero cotangent, which has no sign)
    c["pp"][c["pspec"].logstd:] = np.asarray([0.02, -0.03, 0.01], np.float32).astype(np.float64)
    c["old_logstd"], c["global_step"], h["cov_bound"] = c["pp"][c["pspec"].logstd:].copy(), 1000.0, COV_BOUND
    if not given:       # the rollout's means ARE the incoming policy's: maha is 0 at the first step and well past the bound from the second
        c["old_means"] = np.asarray(nets.forward(c["pspec"], c["pp"], c["states"])[0], np.float32).astype(np.float64)
        h["mean_bound"] = 0.005
    c["logp_old"] = np.asarray(tw.run_case(c)[4]["logp"] + np.random.default_rng(3).uniform(-0.02, 0.02, B), np.float32).astype(np.float64)
    key = L.prng_key(5)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    perm = torch.zeros(E, B, dtype=torch.int32, device=dev)
    ctx.permutation(key.copy(), perm.view(-1), E, B)
    idx = perm.cpu().numpy().reshape(E * M, MB)
    lrs = np.array([3e-3, 2e-3, 1e-3, 5e-4], np.float32)
    ps, cs = ppo.TrainState(c["pspec"], c["pp"]), ppo.TrainState(c["cspec"], c["cp"])
    met, infos = tw.update(ps, cs, c["states"], c["actions"], c["old_means"], c["old_logstd"], c["logp_old"], c["returns"], c["adv"], idx,
                    lrs.astype(np.float64), c["global_step"], h)
    assert all(tw.margins_ok(dict(c, h=h), info) for info in infos) and [i["cov_on"] for i in infos] == [False, True, True, True]
    pd, cd = descs(c)
    p, q = t(c["pp"]), t(c["cp"])
    pm, pv, cm, cv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(q), torch.zeros_like(q)
    out = torch.zeros(E * M, 14, device=dev)
    sh = lambda x: t(x).view(1, B, -1) if np.ndim(x) == 2 else t(x).view(1, B)
    _, count = ctx.dtrl_update(pd, p, pm, pv, cd, q, cm, cv, sh(c["states"]), sh(c["actions"]), sh(c["old_means"]) if given else None,
                               sh(c["logp_old"]), sh(c["returns"]), sh(c["adv"]), E, MB, key, 0, lrs, c["global_step"], hparams(h), out)
    assert count == E * M
    got = out.cpu().numpy().astype(np.float64)
    print("dtrl update metrics, |got - twin| / max(|twin|, 1) per step:\n", np.abs(got - met) / np.maximum(np.abs(met), 1.0), "\ntwin:\n", met)
    assert np.all(np.abs(got - met) <= 1e-5 * np.maximum(np.abs(met), 1.0)), np.abs(got - met).max(0)
    for st, par, m1, m2, p0 in ((ps, p, pm, pv, c["pp"]), (cs, q, cm, cv, c["cp"])):
        n = lambda x: x.cpu().numpy().astype(np.float64)
        sel = np.abs(st.m) > 1e-3 * np.sqrt(np.mean(st.m ** 2))
        figures = (rel(n(par), st.params), rel(n(m1), st.m), rel(n(m2), st.v), rel((n(par) - p0)[sel], (st.params - p0)[sel]))
        print("dtrl update figures:", given, ["%.2e" % v for v in figures])
        assert figures[0] < 1e-5 and figures[1] < 1e-5 and figures[2] < 5e-5 and figures[3] < 2e-4, figures
