"""GPU: one minibatch of PPO-DTRL's loss (rlx_dtrl_loss_f32, rl-x_amd/csrc/dtrl.hip) against the float64 twin (tests/dtrl_twin.py):
the twelve metrics, eta, d logstd, the head seed through the policy gradients, the critic gradients."""
import numpy as np
import pytest
import torch

import dtrl_twin as tw
from rlx_amd.hip import ACT_ELU, DtrlHparams, mlp_desc

pytestmark = pytest.mark.gpu

MODES = {"none": (0, 0, 0), "mean": (1, 0, 0), "cov": (0, 1, 0), "entropy": (0, 0, 1), "all": (1, 1, 1)}
# eta and d logstd have no counterpart in tests/test_gpu_espo.py: the twin in float32 against the twin in float64 on these very
# inputs (all 60 cases) is off by at most 1.54e-6 (eta, relative) and 3.40e-6 (d logstd, L2 relative to max(norm, entropy_coef): at
# A = 1 an active entropy projection makes d logstd exactly zero); 8 x that for reduction order
ETA_TOL = 8 * 1.54e-6
DLOGSTD_TOL = 8 * 3.40e-6


def hparams(h, critic_states=None):
    return DtrlHparams(h["clip_range"], h["entropy_coef"], h["critic_coef"], h["max_grad_norm"], 0.9, 0.999, 1e-8, h["mean_bound"],
                       h["cov_bound"], h["trust_region_coef"], h["total_timesteps"], critic_states)


def descs(c):
    p, q = c["pspec"], c["cspec"]
    return mlp_desc(p.in_dim, p.hidden, p.out_dim, ACT_ELU, True, True), mlp_desc(q.in_dim, q.hidden, 1, ACT_ELU, True, False)


def rel(got, exp):
    return np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30)


@pytest.mark.parametrize("rows", ["smallest", "partial_wave", "two_workgroups"])
@pytest.mark.parametrize("A", [1, 3, 8, 17])
@pytest.mark.parametrize("mode", list(MODES))
def test_loss_matches_the_twin(ctx, dev, mode, A, rows):
    """sub-group widths 1, 4, 8 and 32; the smallest minibatch, the smallest that leaves a partial wave of rows, and one of more than
    one workgroup with a partial wave"""
    W = 1 << (A - 1).bit_length()
    mb = {"smallest": 2, "partial_wave": 64 // W + 1, "two_workgroups": 4 * (64 // W) + 3}[rows]
    c = tw.case(100 + A, A, mb, *MODES[mode])
    _, met, gp, gc, info = tw.run_case(c)
    assert tw.margins_ok(c, info)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    pd, cd = descs(c)
    pg, cg, out = torch.zeros(gp.size, device=dev), torch.zeros(gc.size, device=dev), torch.zeros(12, device=dev)
    ctx.dtrl_loss(pd, t(c["pp"]), pg, cd, t(c["cp"]), cg, t(c["states"]), t(c["actions"]), t(c["old_means"]), t(c["old_logstd"]),
                  t(c["logp_old"]), t(c["returns"]), t(c["adv"]), c["global_step"], hparams(c["h"]), out)
    got, pg, cg = out.cpu().numpy().astype(np.float64), pg.cpu().numpy(), cg.cpu().numpy()
    ls = c["pspec"].logstd
    i_eta = tw.METRICS.index("projection/eta_cov")
    figures = {"metrics": float(np.max(np.abs(got - met) / np.maximum(np.abs(met), 1.0))), "policy": rel(pg[:ls], gp[:ls]),
               "critic": rel(cg, gc), "eta": abs(got[i_eta] - met[i_eta]) / max(met[i_eta], 1e-30),
               "dlogstd": np.linalg.norm(pg[ls:] - gp[ls:]) / max(np.linalg.norm(gp[ls:]), c["h"]["entropy_coef"])}
    print("dtrl figures:", mode, A, mb, {k: "%.2e" % v for k, v in figures.items()})
    assert figures["metrics"] <= 1e-5 and figures["policy"] < 1e-5 and figures["critic"] < 1e-5, figures
    assert figures["dlogstd"] < DLOGSTD_TOL and (figures["eta"] < ETA_TOL if MODES[mode][1] else got[i_eta] == 0.0), figures
