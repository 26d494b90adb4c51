"""CPU: the case table of tests/dtrl_cases.py is fit to pin dtrl.hip -- no rounding decides a branch of any case, the surrogate is
clipped on some rows and not on others, the mixed cases project some rows' means and not others', and the float32 twin holds every bar
of the GPU tests within half, so that what a GPU test finds is the kernel and not the number format."""
import numpy as np
import pytest

import dtrl_cases as dc
import dtrl_twin as tw

I = {k: i for i, k in enumerate(tw.METRICS)}


@pytest.mark.parametrize("name", dc.NAMES)
def test_loss_case_is_decided_by_no_rounding_and_float32_holds_half_the_bars(name):
    k = dc.CASES[name]
    c, (_, met, gp, gc, info) = k.c, k.twin64
    assert k.margins_ok() and info["cov_on"] == k.cov_on and info["ent_on"] == k.ent_on
    assert c["states"].shape == (k.mb, c["pspec"].in_dim) and c["actions"].shape == (k.mb, k.A)
    share = float(np.mean(info["maha"] > c["h"]["mean_bound"]))
    if k.ent_on:        # every ratio inside the clip range (the zero cotangent behind the entropy projection)
        assert met[I["policy_ratio/clip_fraction"]] == 0.0
    else:
        assert 0.1 <= met[I["policy_ratio/clip_fraction"]] <= 0.5
    if k.mixed:
        assert 0.25 <= share <= 0.75
    if k.A > 1 and k.cov_on:
        assert info["d_cov_pred"].shape == (k.mb, k.A) and np.all(np.abs(info["d_cov_pred"]) >= 1e-12)
    _, m32, gp32, gc32, i32 = k.twin32
    assert i32["cov_on"] == info["cov_on"] and i32["ent_on"] == info["ent_on"]
    f = dc.figures(c, m32, gp32, gc32, met, gp, gc)
    print("dtrl case figures (float32 twin):", name, "share %.2f clip %.3f eta %.4g" % (share, met[I["policy_ratio/clip_fraction"]], met[dc.I_ETA]),
          {a: "%.3e" % b for a, b in f.items()})
    assert f["metrics"] <= 0.5 * dc.BAR and f["policy"] <= 0.5 * dc.BAR and f["critic"] <= 0.5 * dc.BAR, f
    assert f["eta"] <= 0.5 * dc.ETA_TOL and f["dlogstd"] <= 0.5 * dc.DLOGSTD_TOL, f
    if not k.cov_on:
        assert m32[dc.I_ETA] == 0.0 and met[dc.I_ETA] == 0.0


def test_the_derived_bars_are_the_tables_own_maxima():
    """ETA_F32_MAX and DLOGSTD_F32_MAX are what the table gives (float32 arithmetic differs a little between CPUs: within a factor 2
    either way, which leaves every case inside half its bar), not figures from other inputs"""
    worst = {"eta": (0.0, None), "dlogstd": (0.0, None)}
    for name, k in dc.CASES.items():
        f = dc.figures(k.c, *k.twin32[1:4], *k.twin64[1:4])
        for key in worst:
            if f[key] > worst[key][0]:
                worst[key] = (f[key], name)
    print("dtrl derived bars:", worst)
    assert 0.5 * dc.ETA_F32_MAX <= worst["eta"][0] <= 2.0 * dc.ETA_F32_MAX
    assert 0.5 * dc.DLOGSTD_F32_MAX <= worst["dlogstd"][0] <= 2.0 * dc.DLOGSTD_F32_MAX


def test_the_table_reaches_what_it_is_for():
    """the sub-group widths, the loop trips and the buffers each group of cases exists for (dtrl.hip's constants restated)"""
    width = lambda A: 1 << (A - 1).bit_length()
    assert {width(k.A) for k in dc.CASES.values()} >= {2, 16, 64} and {k.A for k in dc.CASES.values()} >= {16, 33, 64}
    k = dc.CASES["rows2_4100"]
    assert k.mb > 1024 * 256 // width(k.A) and width(k.A) == 64          # DT_MAX_BLOCKS * 256 / W rows per pass
    assert all(dc.CASES[n].mb > 1024 for n in ("adv_1025", "adv_1100", "adv_1025_ce", "adv_1100_ce"))
    assert [(-dc.CASES[n].c["pspec"].in_dim) % 4 for n in ("in_1", "in_5", "in_6")] == [3, 3, 2]
    for n, (op, oc) in {"cs_wide": (5, 11), "cs_narrow": (9, 4), "cs_same": (7, 7)}.items():
        c = dc.CASES[n].c
        assert (c["pspec"].in_dim, c["cspec"].in_dim) == (op, oc) and c["cstates"].shape == (dc.CASES[n].mb, oc)
    assert not np.array_equal(dc.CASES["cs_same"].c["cstates"], dc.CASES["cs_same"].c["states"])
    for n in ("negH_3_on", "negH_8_on", "negH_3_off", "negH_8_off"):
        info = dc.CASES[n].twin64[4]
        assert info["beta"] < 0 and info["ent_on"] == n.endswith("_on") and dc.CASES[n].c["global_step"] == 370.0
    assert dc.CASES["cov_1e4"].twin64[1][dc.I_ETA] > 100 and 0 < dc.CASES["cov_2"].twin64[1][dc.I_ETA] < 1


@pytest.mark.parametrize("name", list(dc.UPDATES))
def test_update_case_is_decided_by_no_rounding(name):
    u = dc.UPDATES[name]
    b = u.built
    met, infos, ps, cs = b["twin"]
    c = b["c"]
    assert b["idx"].shape == (u.n_upd, u.mb) and all(sorted(e) == list(range(u.B)) for e in b["idx"].reshape(u.E, u.B))
    assert ps.count == cs.count == u.opt_count0 + u.n_upd
    if u.poison:        # a non-finite row: only the untouched side is compared (the twin's optimiser does not skip)
        bad = met[0, 13 if u.poison == "returns" else 12]
        good = met[0, 12 if u.poison == "returns" else 13]
        assert not np.isfinite(bad) and np.isfinite(good) and good > 0
        return
    assert all(tw.margins_ok(c, info) for info in infos) and [i["cov_on"] for i in infos] == dc.UPDATE_COV_ON(u)
    assert not any(i["ent_on"] for i in infos) and np.all(np.isfinite(met))
    if u.opt_count0:
        assert np.abs(b["start"][1]).max() > 0 and np.abs(b["start"][4]).max() > 0 and b["start"][2].min() >= 0
    if u.clip:          # both networks clipped at every step
        assert np.all(met[:, 12:14] > 1.5 * c["h"]["max_grad_norm"])
    else:
        assert np.all(met[:, 12:14] < c["h"]["max_grad_norm"])
