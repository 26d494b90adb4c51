"""GPU: rlx_dtrl_loss_f32 (rl-x_amd/csrc/dtrl.hip) against the float64 twin over the case table of tests/dtrl_cases.py -- the
sub-group widths 2, 16 and 64, rows of one wave on both sides of the mean bound, the second pass of the row loop and of the advantage
statistics, every network shape dt_check_desc takes, hp->critic_states, the covariance step at a distant and a near bound, a negative
entropy bound -- with test_gpu_dtrl.py's comparisons and bars; that two identical calls give identical bits; and that what the host
checks refuse is refused before anything is written."""
import numpy as np
import pytest
import torch

import dtrl_cases as dc
from rlx_amd.hip import lib as L
from rlx_amd.hip import mlp_desc
from test_gpu_dtrl import hparams

pytestmark = pytest.mark.gpu


def descs(c):
    """test_gpu_dtrl.py's descs with the case's own activation and LayerNorm flag"""
    p, q = c["pspec"], c["cspec"]
    return mlp_desc(p.in_dim, p.hidden, p.out_dim, p.act, p.ln_first, True), mlp_desc(q.in_dim, q.hidden, 1, q.act, q.ln_first, False)


def run_loss(ctx, dev, c, fill=0.0):
    """-> (metrics [12], policy gradient, critic gradient) of one call, as float32 arrays"""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    pd, cd = descs(c)
    pg, cg = torch.full((c["pspec"].n_params,), fill, device=dev), torch.full((c["cspec"].n_params,), fill, device=dev)
    out = torch.full((12,), fill, device=dev)
    cst = None if c["cstates"] is None else t(c["cstates"])     # (alive until the results are read)
    ctx.dtrl_loss(pd, t(c["pp"]), pg, cd, t(c["cp"]), cg, t(c["states"]), t(c["actions"]), t(c["old_means"]), t(c["old_logstd"]),
                  t(c["logp_old"]), t(c["returns"]), t(c["adv"]), c["global_step"], hparams(c["h"], None if cst is None else cst.data_ptr()),
                  out)
    return out.cpu().numpy(), pg.cpu().numpy(), cg.cpu().numpy()


@pytest.mark.parametrize("name", dc.NAMES)
def test_loss_matches_the_twin_over_the_table(ctx, dev, name):
    k = dc.CASES[name]
    c, (_, met, gp, gc, info) = k.c, k.twin64
    assert k.margins_ok()
    got, pg, cg = run_loss(ctx, dev, c, fill=7.0)       # (every output is written whole: nothing of the fill may remain)
    f = dc.figures(c, got, pg, cg, met, gp, gc)
    print("dtrl shape figures:", name, k.A, k.mb, {a: "%.2e" % b for a, b in f.items()})
    assert f["metrics"] <= dc.BAR and f["policy"] < dc.BAR and f["critic"] < dc.BAR, f
    assert f["dlogstd"] < dc.DLOGSTD_TOL and (f["eta"] < dc.ETA_TOL if k.cov_on else got[dc.I_ETA] == 0.0), f


@pytest.mark.parametrize("name", dc.REPEAT_NAMES)
def test_two_identical_calls_give_identical_bits(ctx, dev, name):
    """dtrl.hip's header: every reduction has a fixed order, no atomics"""
    c = dc.CASES[name].c
    first, second = run_loss(ctx, dev, c), run_loss(ctx, dev, c, fill=3.0)
    for a, b, what in zip(first, second, ("metrics", "policy gradient", "critic gradient")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    assert np.all(np.isfinite(first[0])) and np.abs(first[1]).max() > 0 and np.abs(first[2]).max() > 0


def refused_call(c, change):
    """the descs, hparams and rows of a small accepted case with one refusal's change applied -> (pd, cd, hp, mb)"""
    p, q, h = c["pspec"], c["cspec"], dict(c["h"])
    d = {"p": dict(in_dim=p.in_dim, hidden=tuple(p.hidden), out_dim=p.out_dim, act=p.act, ln_first=1, has_logstd=1),
         "c": dict(in_dim=q.in_dim, hidden=tuple(q.hidden), out_dim=1, act=q.act, ln_first=1, has_logstd=0)}
    extra = {}
    for key, v in change.items():
        if key[:2] in ("p.", "c."):
            d[key[0]][key[2:]] = v
        elif key[:2] == "h.":
            h[key[2:]] = v
        else:
            extra[key] = v
    mk = lambda a: mlp_desc(a["in_dim"], a["hidden"], a["out_dim"], a["act"], a["ln_first"], a["has_logstd"])
    return mk(d["p"]), mk(d["c"]), hparams(h), extra


REFUSAL_BASE = "in_5"       # A = 3, 9 rows, obs 5: small, accepted, and run by the table above


@pytest.mark.parametrize("name", list(dc.REFUSED))
def test_loss_refuses_what_its_checks_refuse(ctx, dev, name):
    change, code, field = dc.REFUSED[name]
    c = dc.CASES[REFUSAL_BASE].c
    pd, cd, hp, extra = refused_call(c, change)
    mb = extra.get("mb", c["actions"].shape[0])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    n = 1 << 20                                         # (room for the parameters of any refused shape)
    pp, cp, pg, cg = (torch.full((n,), 7.0, device=dev) for _ in range(4))
    out = torch.full((12,), 7.0, device=dev)
    with pytest.raises(L.RlxError) as e:
        ctx.dtrl_loss(pd, pp, pg, cd, cp, cg, t(c["states"]), t(c["actions"][:mb]), t(c["old_means"]), t(c["old_logstd"]), t(c["logp_old"]),
                      t(c["returns"]), t(c["adv"]), c["global_step"], hp, out)
    torch.cuda.synchronize()
    assert "rc=%d)" % code in str(e.value) and field in str(e.value) and "rlx_dtrl_loss_f32" in str(e.value), str(e.value)
    assert bool((pg == 7.0).all()) and bool((cg == 7.0).all()) and bool((out == 7.0).all())
    # the context serves an accepted call after the refusal
    k = dc.CASES[REFUSAL_BASE]
    got, gpol, gcri = run_loss(ctx, dev, c)
    f = dc.figures(c, got, gpol, gcri, *k.twin64[1:4])
    assert f["metrics"] <= dc.BAR and f["policy"] < dc.BAR and f["critic"] < dc.BAR, f
