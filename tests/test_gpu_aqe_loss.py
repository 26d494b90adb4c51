"""GPU: rlx_aqe_losses_f32 -- AQE's truncated-mean target, critic loss / gradient (k_aqe_target_loss) and the policy's constant seed
and row means on given values -- against the float64 twin (tests/aqe_twin.py).  The library's Q arrays are [E, B, H], the twin's
[B, T] with column e H + h.

Bars: y within 1e-6 of the magnitude of its terms, |r| + gamma (1 - term) (max |q'| + alpha |logp'|), per row (tests/test_gpu_tqc_loss.py's
rule: a sum that can cancel is no scale for itself); the loss and dq at 1e-6 relative L2 (tests/test_gpu_redq_loss.py's).  The twin
evaluated in numpy float32 on the same inputs is itself off the float64 twin by F32_GAP below (measured once on a CPU: this file
run as a script, repository root and rl-x_amd on PYTHONPATH); a case is held to twice that gap where that exceeds its bar."""
import numpy as np
import pytest
import torch

import aqe_twin as tw

pytestmark = pytest.mark.gpu

GAMMA = 0.99
BAR = 1e-6
SHAPES = [(1, 1, 0), (2, 1, 1), (10, 2, 4), (3, 5, 14), (16, 4, 0), (13, 5, 7), (16, 8, 100)]
ROWS = [1, 13, 257]
# (y, dq, loss) figures of the numpy float32 twin against the float64 twin, the largest over B in ROWS per shape.  Twice every gap is
# below the 1e-6 bar: all 21 cases meet the bars as stated.
F32_GAP = {
    (1, 1, 0): (9.3e-08, 6.2e-08, 1.0e-07),
    (2, 1, 1): (7.5e-08, 5.5e-08, 8.9e-08),
    (10, 2, 4): (6.2e-08, 4.9e-08, 6.6e-08),
    (3, 5, 14): (1.0e-07, 5.3e-08, 7.7e-08),
    (16, 4, 0): (5.1e-08, 4.6e-08, 1.5e-08),
    (13, 5, 7): (4.3e-08, 4.8e-08, 3.4e-08),
    (16, 8, 100): (1.1e-07, 6.2e-08, 4.9e-08),
}


def _hp(E, H, dropped, G=1):
    from rlx_amd.hip import AqeHparams
    return AqeHparams(GAMMA, 0.005, -1.0, -20.0, 2.0, 3e-4, 3e-4, 0.0, 3e-4, 0.9, 0.999, 1e-8, E, H, dropped, G)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _lib(x, E, H):
    """twin [B, T] -> library [E, B, H]"""
    return np.ascontiguousarray(x.reshape(x.shape[0], E, H).transpose(1, 0, 2))


def _twin(x, E, H):
    """library [E, B, H] -> twin [B, T]"""
    return np.asarray(x).transpose(1, 0, 2).reshape(x.shape[1], E * H)


def _inputs(B, E, H, seed):
    """all Q arrays in the twin's [B, T] layout"""
    rng = np.random.default_rng(seed)
    T = E * H
    f = lambda x: x.astype(np.float32)
    term = f(rng.random(B) < 0.3)
    term[0] = 1.0                                                      # at least one terminated row: y = r exactly
    return dict(q=f(rng.standard_normal((B, T))), qn=f(rng.standard_normal((B, T))), r=f(rng.standard_normal(B)), term=term,
                nlogp=f(rng.standard_normal(B)), la=np.array([-0.3], np.float32), qa=f(rng.standard_normal((B, T))))


def _expect(x, K, dtype=np.float64):
    c = lambda v: v.astype(dtype)
    return tw.critic_loss(c(x["q"]), c(x["qn"]), c(x["r"]), c(x["term"]), np.exp(c(x["la"])[0]), c(x["nlogp"]), dtype(GAMMA), K)


def _figures(x, y, dq, loss, K):
    """(y, dq, loss) of an evaluation against the float64 twin: the largest row error of y over the magnitude of its terms, relative
    L2 of dq [B, T], relative error of the loss"""
    y_e, loss_e, dq_e = _expect(x, K)
    f8 = lambda v: np.asarray(v, np.float64)
    alpha = np.exp(np.float64(x["la"][0]))
    scale = np.abs(f8(x["r"])) + GAMMA * (1 - f8(x["term"])) * (np.abs(f8(x["qn"])).max(axis=1) + alpha * np.abs(f8(x["nlogp"])))
    rel = lambda got, exp: float(np.linalg.norm(f8(got) - exp) / max(np.linalg.norm(exp), 1e-30))
    return (float((np.abs(f8(y) - y_e) / np.maximum(scale, 1e-30)).max()), rel(dq, dq_e), abs(float(loss) - loss_e.mean()) / loss_e.mean())


def f32_gap(E, H, dropped):
    out = np.zeros(3)
    for B in ROWS:
        x = _inputs(B, E, H, 100 * B + 7 * E + H)
        y, loss, dq = _expect(x, E * H - dropped, np.float32)
        assert y.dtype == np.float32 and dq.dtype == np.float32
        out = np.maximum(out, _figures(x, y, dq, loss.mean(), E * H - dropped))
    return tuple(out)


def _run(ctx, dev, x, E, H, dropped, with_y=True, with_policy=True):
    B, T = x["q"].shape
    d = {k: _t(_lib(v, E, H) if v.ndim == 2 else v, dev) for k, v in x.items()}
    full = lambda *s: torch.full(s, 7.0, device=dev)
    o = dict(y=full(B) if with_y else None, dq=full(E, B, H), loss=full(1), seed=full(E, B, H) if with_policy else None,
             meanq=full(B) if with_policy else None)
    ctx.aqe_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, H, dropped), o["dq"], o["y"], o["loss"],
                   d["qa"] if with_policy else None, o["seed"], o["meanq"])
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("E,H,dropped", SHAPES)
@pytest.mark.parametrize("B", ROWS)
def test_losses_match_twin(ctx, dev, B, E, H, dropped):
    T, K = E * H, E * H - dropped
    x = _inputs(B, E, H, 100 * B + 7 * E + H)
    o = _run(ctx, dev, x, E, H, dropped)
    fig = _figures(x, o["y"], _twin(o["dq"], E, H), o["loss"][0], K)
    gap = F32_GAP.get((E, H, dropped), (0.0, 0.0, 0.0))
    bars = tuple(max(BAR, 2 * g) for g in gap)
    print(f"aqe losses B={B} E={E} H={H} dropped={dropped}: y {fig[0]:.1e}/{bars[0]:.1e} dq {fig[1]:.1e}/{bars[1]:.1e} "
          f"loss {fig[2]:.1e}/{bars[2]:.1e}")
    assert all(f <= b for f, b in zip(fig, bars)), (fig, bars)
    done = x["term"] == 1.0
    assert done.any() and np.array_equal(o["y"][done], x["r"][done])                  # terminated rows: y = r exactly
    # the policy's head: the seed is exactly -1 / (B T) everywhere; the row mean of T float32 values in a fixed-order tree of at most
    # 7 levels is within 7 * 2^-24 max|qa| < 1e-6 max|qa| of the exact one
    assert np.array_equal(o["seed"], np.full((E, B, H), np.float32(-1.0) / (np.float32(B) * np.float32(T)), np.float32))
    mean_e, _ = tw.policy_seed(x["qa"].astype(np.float64))
    assert np.all(np.abs(o["meanq"] - mean_e) <= 1e-6 * np.abs(x["qa"]).max(axis=1))


@pytest.mark.parametrize("E,H,dropped", [(3, 2, 2), (16, 4, 10), (13, 5, 7), (16, 8, 100)])
def test_sorted_reversed_and_duplicate_rows(ctx, dev, E, H, dropped):
    """B = 5 hand-shaped target rows: ascending, descending, all equal, duplicates straddling the cut (the value at sorted position
    K - 1 repeated on both sides of it), and -- with every row terminated in a second call -- y = r exactly"""
    T, K, B = E * H, E * H - dropped, 5
    x = _inputs(B, E, H, 31 + T)
    x["term"][:] = 0.0
    asc = (np.arange(T, dtype=np.float32) - T // 3) / 4                # multiples of 1/4: exact in float32
    x["qn"][0] = asc
    x["qn"][1] = asc[::-1]
    x["qn"][2] = 0.75
    dup = asc.copy()
    dup[max(K - 2, 0):min(K + 2, T)] = asc[K - 1]
    x["qn"][3] = np.random.default_rng(T).permutation(dup)
    x["qn"][4] = np.random.default_rng(T + 1).permutation(asc)
    o = _run(ctx, dev, x, E, H, dropped)
    fig = _figures(x, o["y"], _twin(o["dq"], E, H), o["loss"][0], K)
    print(f"aqe losses shaped rows E={E} H={H} dropped={dropped}: y {fig[0]:.1e} dq {fig[1]:.1e} loss {fig[2]:.1e}")
    assert all(f <= BAR for f in fig), fig
    # rows 0, 1 and 4 hold the same multiset: one sorted order, one sum order, the same bits whatever the arrangement
    x1 = dict(x, r=np.zeros(B, np.float32), nlogp=np.zeros(B, np.float32))
    o1 = _run(ctx, dev, x1, E, H, dropped)
    assert o1["y"][0] == o1["y"][1] == o1["y"][4]
    assert o1["y"][2] == np.float32(GAMMA) * np.float32(0.75)
    x2 = dict(x, term=np.ones(B, np.float32))
    assert np.array_equal(_run(ctx, dev, x2, E, H, dropped)["y"], x["r"])


def test_identical_bits_and_null_outputs(ctx, dev):
    E, H, dropped, B = 13, 5, 7, 257
    x = _inputs(B, E, H, 5)
    a, b = _run(ctx, dev, x, E, H, dropped), _run(ctx, dev, x, E, H, dropped)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c = _run(ctx, dev, x, E, H, dropped, with_y=False, with_policy=False)
    assert np.array_equal(c["dq"], a["dq"]) and np.array_equal(c["loss"], a["loss"]) and c["loss"][0] > 0
    # loss_out may be NULL as well: dq alone
    d = {k: _t(_lib(v, E, H) if v.ndim == 2 else v, dev) for k, v in x.items()}
    dq = torch.zeros(E, B, H, device=dev)
    ctx.aqe_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, H, dropped), dq)
    assert np.array_equal(dq.cpu().numpy(), a["dq"])
    # seed without meanq
    seed = torch.zeros(E, B, H, device=dev)
    ctx.aqe_losses(d["q"], d["qn"], d["r"], d["term"], d["nlogp"], d["la"], _hp(E, H, dropped), dq, qa=d["qa"], seed_out=seed)
    assert np.array_equal(seed.cpu().numpy(), a["seed"])


@pytest.mark.parametrize("what,code,word", [
    ("e0", -1, "ensemble_size"), ("e17", -4, "ensemble_size"), ("h0", -1, "nr_heads_per_net"), ("t129", -4, "at most 128"),
    ("dropped_t", -1, "nr_dropped_q_values"), ("dropped_neg", -1, "nr_dropped_q_values"), ("g0", -1, "q_update_steps"),
    ("g65", -4, "q_update_steps"), ("no_seed", -1, "seed_out"), ("no_dq", -1, "dq_out"), ("no_q", -1, "NULL input")])
def test_refusals_leave_the_outputs_alone(ctx, dev, what, code, word):
    from rlx_amd.hip import RlxError
    E, H, dropped, G = 3, 2, 2, 1
    if what == "e0":
        E = 0
    elif what == "e17":
        E = 17
    elif what == "h0":
        H = 0
    elif what == "t129":
        E, H = 3, 43
    elif what == "dropped_t":
        dropped = 6
    elif what == "dropped_neg":
        dropped = -1
    elif what == "g0":
        G = 0
    elif what == "g65":
        G = 65
    B = 8
    x = torch.zeros(4096, device=dev)
    out = torch.full((4096,), 7.0, device=dev)
    kw = dict(y_out=out, loss_out=out, qa=x, seed_out=None if what == "no_seed" else out, meanq_out=out)
    with pytest.raises(RlxError) as e:
        ctx.aqe_losses(None if what == "no_q" else x, x, x[:B], x[:B], x[:B], x[:1], _hp(E, H, dropped, G), None if what == "no_dq" else out, **kw)
    assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()


if __name__ == "__main__":      # the float32 gaps behind F32_GAP (CPU only)
    for s in SHAPES:
        print(f"    {s}: (" + ", ".join(f"{v:.1e}" for v in f32_gap(*s)) + "),")
