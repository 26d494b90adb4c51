"""GPU: the two small entry points of droq.hip.

rlx_droq_mask_u8 -- the library's dropout mask stream -- against its Python restatement (tests/droq_twin.py: mask_stream, built from
oracle/prng.py's split, random_bits and uniform alone), bit for bit.

rlx_droq_block_f32 -- the fused Dropout -> LayerNorm -> ReLU kernel, forward and backward -- against the twin's block in float64 on
the same float32 inputs and the Python mask.  D: one lane group (64), the lean form's edge (256), just past it (320), the wide form's
edge (768); M: fewer rows than a workgroup holds (1, 3), a ragged last workgroup (5, 67); rate 0 (no draws), 0.01, 0.25, 0.9.

Bars: each output (H, dZ, d scale, d bias) is held to the larger of 1e-6 relative L2 (tests/test_gpu_redq_loss.py's bar) and twice
F32_GAP, the gap of the same block evaluated in numpy float32 against float64 (measured once on a CPU: this file run as a script,
repository root, tests and rl-x_amd on PYTHONPATH; its output is the SEEDS and F32_GAP tables below).

Every case's inputs come from SEEDS[case]: the first seed for which (asserted again by the test, on the CPU) the case's mask has kept
and dropped units with a dropped share within a factor two of the rate, and no unit's pre-activation lies within KINK of the ReLU's
kink in float64 -- a unit that close may legitimately come out on the other side in float32, which changes its whole row of dZ."""
import numpy as np
import pytest
import torch

import droq_twin as tw
from oracle import prng

pytestmark = pytest.mark.gpu

DS, MS, RATES = (64, 256, 320, 768), (1, 3, 5, 67), (0.0, 0.01, 0.25, 0.9)
KINK = 1e-5
BAR = 1e-6
OUTS = ("H", "dZ", "dg", "db")
J, E, LAYER, L = 1, 2, 1, 2

# (D, M, rate) -> seed (0 where not listed): python tests/test_gpu_droq_block.py
SEEDS = {(D, M, rate): 0 for D in DS for M in MS for rate in RATES}
SEEDS.update({(64, 3, 0.01): 1, (64, 67, 0.25): 2, (256, 5, 0.01): 1, (320, 67, 0.0): 4, (320, 67, 0.9): 2, (768, 67, 0.01): 1, (768, 5, 0.9): 3, (768, 67, 0.9): 5})
# (D, rate) -> {M: (H, dZ, dg, db)}: relative L2 of the float32 block against the float64 one, same inputs and mask.  Every gap is
# below 2e-7: twice it is below the 1e-6 bar, which therefore holds in every case
F32_GAP = {
    (64, 0.0): {1: (6.56e-08, 3.89e-08, 6.21e-08, 0.0), 3: (6.47e-08, 6.99e-08, 6.12e-08, 2.33e-08), 5: (6.31e-08, 6.13e-08, 5.59e-08, 2.98e-08), 67: (7.09e-08, 7.11e-08, 1.15e-07, 1.06e-07)},
    (64, 0.01): {1: (6.09e-08, 7.53e-08, 5.94e-08, 0.0), 3: (1.11e-07, 1.16e-07, 6.93e-08, 2.48e-08), 5: (7.08e-08, 7.21e-08, 7.81e-08, 2.9e-08), 67: (7.34e-08, 7.64e-08, 1.24e-07, 1.15e-07)},
    (64, 0.25): {1: (9.61e-08, 9.42e-08, 9.89e-08, 0.0), 3: (6.64e-08, 7.36e-08, 7.6e-08, 1.93e-08), 5: (8.76e-08, 8.24e-08, 7.57e-08, 2.69e-08), 67: (7.09e-08, 7.61e-08, 1.2e-07, 9.79e-08)},
    (64, 0.9): {1: (1.05e-07, 1.61e-07, 7.93e-08, 0.0), 3: (8.9e-08, 9.65e-08, 8.24e-08, 2.85e-08), 5: (8.76e-08, 8.88e-08, 7.25e-08, 3.27e-08), 67: (7.44e-08, 1.14e-07, 1.03e-07, 1.49e-07)},
    (256, 0.0): {1: (5.18e-08, 6.66e-08, 4.75e-08, 0.0), 3: (6.18e-08, 6.96e-08, 5.7e-08, 2.26e-08), 5: (6.52e-08, 7.03e-08, 6.83e-08, 4e-08), 67: (7.01e-08, 7.2e-08, 1.37e-07, 9.96e-08)},
    (256, 0.01): {1: (6.25e-08, 7.31e-08, 6.27e-08, 0.0), 3: (6.71e-08, 7.58e-08, 6.6e-08, 2.28e-08), 5: (7.02e-08, 6.69e-08, 8.54e-08, 4.03e-08), 67: (7.68e-08, 7.62e-08, 1.24e-07, 9.71e-08)},
    (256, 0.25): {1: (9.01e-08, 9.84e-08, 9.73e-08, 0.0), 3: (5.28e-08, 6.17e-08, 5e-08, 2.36e-08), 5: (7.01e-08, 6.64e-08, 7.91e-08, 3.76e-08), 67: (7.1e-08, 7.09e-08, 1.18e-07, 1.14e-07)},
    (256, 0.9): {1: (8.52e-08, 9.5e-08, 1.41e-07, 0.0), 3: (8.1e-08, 5.8e-08, 6.34e-08, 2.25e-08), 5: (4.92e-08, 6.58e-08, 7.66e-08, 4.07e-08), 67: (8.19e-08, 9.2e-08, 1.01e-07, 1.17e-07)},
    (320, 0.0): {1: (7.4e-08, 7.33e-08, 6.85e-08, 0.0), 3: (8.04e-08, 7.82e-08, 7.68e-08, 2.72e-08), 5: (6.12e-08, 5.56e-08, 6.73e-08, 3.42e-08), 67: (6.8e-08, 6.96e-08, 1.29e-07, 1.02e-07)},
    (320, 0.01): {1: (5.78e-08, 4.79e-08, 5.06e-08, 0.0), 3: (6.97e-08, 6.76e-08, 7.07e-08, 2.71e-08), 5: (6.35e-08, 7.04e-08, 6.85e-08, 3.42e-08), 67: (7.29e-08, 7.18e-08, 1.43e-07, 1.11e-07)},
    (320, 0.25): {1: (6.69e-08, 5.29e-08, 5e-08, 0.0), 3: (6.07e-08, 5.79e-08, 5.82e-08, 2.34e-08), 5: (7.96e-08, 8.12e-08, 9.27e-08, 3.33e-08), 67: (7.09e-08, 6.92e-08, 1.17e-07, 1.02e-07)},
    (320, 0.9): {1: (9.24e-08, 8.69e-08, 4.56e-08, 0.0), 3: (5.86e-08, 7.02e-08, 7.5e-08, 2.42e-08), 5: (5.97e-08, 6.66e-08, 5.11e-08, 3.21e-08), 67: (7.3e-08, 7.6e-08, 9.77e-08, 1.14e-07)},
    (768, 0.0): {1: (8.78e-08, 8.26e-08, 8.77e-08, 0.0), 3: (5.41e-08, 5.5e-08, 5.39e-08, 2.3e-08), 5: (7.77e-08, 7.92e-08, 7.74e-08, 3.43e-08), 67: (6.96e-08, 7.03e-08, 1.3e-07, 1.08e-07)},
    (768, 0.01): {1: (5.72e-08, 5.52e-08, 5.03e-08, 0.0), 3: (6.38e-08, 6.4e-08, 6.6e-08, 2.3e-08), 5: (6.4e-08, 6.06e-08, 6.99e-08, 3.41e-08), 67: (7.58e-08, 7.33e-08, 1.32e-07, 1.09e-07)},
    (768, 0.25): {1: (7.27e-08, 4.95e-08, 6.19e-08, 0.0), 3: (7.32e-08, 7.83e-08, 7.31e-08, 2.23e-08), 5: (6.99e-08, 6.93e-08, 6.8e-08, 3.28e-08), 67: (7.52e-08, 7.44e-08, 1.12e-07, 9.48e-08)},
    (768, 0.9): {1: (8.17e-08, 8.11e-08, 6.98e-08, 0.0), 3: (5.7e-08, 6.05e-08, 4.5e-08, 3.13e-08), 5: (6.93e-08, 8.49e-08, 7.29e-08, 3.94e-08), 67: (7.78e-08, 8.16e-08, 1.15e-07, 1.25e-07)},
}


def _rel(got, exp):
    return float(np.linalg.norm(np.asarray(got, np.float64) - exp) / max(np.linalg.norm(exp), 1e-30))


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def scheme_of(D, M):
    """both threefry schemes reach the kernel: the legacy one on every other case"""
    return (DS.index(D) + MS.index(M)) % 2


def make_case(D, M, rate, seed):
    """-> dict(key, layout, mask, Z, gb, dY) of float32 inputs and the Python mask"""
    rng = np.random.default_rng([seed, D, M])
    key = prng.prng_key(1000 + seed)
    layout = tw.LAYOUTS["online"](M)
    mask = tw.mask_stream(key, layout, J, E, LAYER, L, M, D, rate, bool(scheme_of(D, M)))
    f = lambda x: x.astype(np.float32)
    return dict(key=key, layout=layout, mask=mask, Z=f(1.5 * rng.standard_normal((M, D)) + 0.3),
                gb=f(np.concatenate([1.0 + 0.1 * rng.standard_normal(D), 0.1 * rng.standard_normal(D)])), dY=f(rng.standard_normal((M, D))))


def twin_block(c, D, rate, dtype=np.float64):
    Z, gb, dY = (c[k].astype(dtype) for k in ("Z", "gb", "dY"))
    H, cache = tw.block_forward(Z, c["mask"], tw.keep_prob(rate), gb[:D], gb[D:])
    dZ, dg, db = tw.block_backward(dY, cache)
    pre = cache["xhat"] * gb[:D] + gb[D:]
    return {"H": H, "dZ": dZ, "dg": dg, "db": db}, pre


def case_is_usable(c, D, rate):
    """the conditions of the module docstring, on the CPU"""
    dropped = float((~c["mask"]).mean())
    if rate > 0 and not (c["mask"].any() and (~c["mask"]).any() and rate / 2 <= dropped <= 2 * rate):
        return False
    if rate == 0 and not c["mask"].all():
        return False
    exp, pre = twin_block(c, D, rate)
    return float(np.abs(pre).min()) > KINK and bool(np.all(exp["dZ"][c["mask"]] != 0))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("D", DS)
def test_block_forward_and_backward_match_the_twin(ctx, dev, D, rate):
    for M in MS:
        seed = SEEDS[(D, M, rate)]
        c = make_case(D, M, rate, seed)
        assert case_is_usable(c, D, rate), (D, M, rate, seed)
        scheme = scheme_of(D, M)
        exp, _ = twin_block(c, D, rate)
        Z, gb = _t(c["Z"], dev), _t(c["gb"], dev)
        Z0 = Z.clone()
        H = torch.full((M, D), 7.0, device=dev)
        ctx.droq_block(Z, H, gb, c["key"], c["layout"], J, E, LAYER, L, rate, scheme)
        dZ, dg, db = _t(c["dY"], dev), torch.full((D,), 7.0, device=dev), torch.full((D,), 7.0, device=dev)
        ctx.droq_block(Z, dZ, gb, c["key"], c["layout"], J, E, LAYER, L, rate, scheme, dg_out=dg, db_out=db)
        torch.cuda.synchronize()
        assert torch.equal(Z, Z0)                                                   # Z stays pre-dropout: nothing else is written
        got = {"H": H.cpu().numpy(), "dZ": dZ.cpu().numpy(), "dg": dg.cpu().numpy(), "db": db.cpu().numpy()}
        gap = F32_GAP[(D, rate)][M]
        fig = {k: _rel(got[k], exp[k]) for k in OUTS}
        bars = {k: max(BAR, 2 * gap[i]) for i, k in enumerate(OUTS)}
        print(f"droq block D={D} M={M} rate={rate} scheme={scheme}: " + " ".join(f"{k} {fig[k]:.2e}/{bars[k]:.1e}" for k in OUTS))
        bad = {k: (fig[k], bars[k]) for k in OUTS if not fig[k] <= bars[k]}
        assert not bad, (D, M, rate, bad)
        # dropped units give exactly 0 in dZ, and the backward's regenerated mask is the forward's: dZ is non-zero exactly on the
        # mask the forward's H was checked under (a kept unit's dZ is a sum of continuous terms: never exactly 0)
        assert np.array_equal(got["dZ"] != 0, c["mask"]), (D, M, rate)
        assert not np.any(got["dZ"][~c["mask"]])
        # two calls give identical bits
        H2, dZ2, dg2, db2 = torch.empty_like(H), _t(c["dY"], dev), torch.empty_like(dg), torch.empty_like(db)
        ctx.droq_block(Z, H2, gb, c["key"], c["layout"], J, E, LAYER, L, rate, scheme)
        ctx.droq_block(Z, dZ2, gb, c["key"], c["layout"], J, E, LAYER, L, rate, scheme, dg_out=dg2, db_out=db2)
        assert torch.equal(H, H2) and torch.equal(dZ, dZ2) and torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize("D", [256, 320])
def test_forward_mask_is_the_backward_mask(ctx, dev, D):
    """a designed input shows the FORWARD's mask by itself: Z = 4 everywhere, scale 1, bias 0 -> a kept unit is 4 / keep, above its
    row's mean, and comes out positive; a dropped one is 0, below it, and comes out 0.  The backward of a random dY on a random Z
    under the same keys is zero exactly on the dropped units.  Both equal the mask entry point's flags and the Python mask"""
    M, rate, key = 67, 0.25, prng.prng_key(77)
    layout = tw.LAYOUTS["policy"](M)
    mask = tw.mask_stream(key, layout, 0, E, 0, L, M, D, rate)
    assert (mask.any(axis=1) & (~mask).any(axis=1)).all()
    gb = _t(np.concatenate([np.ones(D), np.zeros(D)]), dev)
    H = torch.empty((M, D), device=dev)
    ctx.droq_block(torch.full((M, D), 4.0, device=dev), H, gb, key, layout, 0, E, 0, L, rate)
    rng = np.random.default_rng(5)
    Z, dZ = _t(rng.standard_normal((M, D)), dev), _t(rng.standard_normal((M, D)), dev)
    ctx.droq_block(Z, dZ, gb, key, layout, 0, E, 0, L, rate, dg_out=torch.empty(D, device=dev), db_out=torch.empty(D, device=dev))
    flags = ctx.droq_mask(key, layout, 0, E, 0, L, M, D, rate).cpu().numpy().astype(bool)
    fwd, bwd = (H > 0).cpu().numpy(), (dZ != 0).cpu().numpy()
    assert np.array_equal(fwd, mask) and np.array_equal(bwd, mask) and np.array_equal(flags, mask)


def mask_cases():
    """both schemes x the three key layouts x E in {1, 2, 16} with EVERY j; L in {1, 3} with every l, D in {64, 192, 768}, B in {1, 67}
    and the rates cycle underneath so that every value meets every scheme and layout"""
    out, i = [], 0
    for scheme in (1, 0):
        for name in ("online", "target", "policy"):
            for E_ in (1, 2, 16):
                for j in range(E_):
                    L_, l = ((1, 0), (3, 0), (3, 1), (3, 2))[i % 4]
                    out.append((scheme, name, E_, j, L_, l, (64, 192, 768)[i % 3], (1, 67)[(i // 2) % 2], (0.25, 0.01, 0.9)[(i // 3) % 3]))
                    i += 1
    return out


def test_mask_equals_the_python_restatement(ctx, dev):
    cases = mask_cases()
    for scheme in (1, 0):
        for name in ("online", "target", "policy"):
            seen = [c for c in cases if c[0] == scheme and c[1] == name]
            assert {(c[4], c[5]) for c in seen} == {(1, 0), (3, 0), (3, 1), (3, 2)} and {c[6] for c in seen} == {64, 192, 768}
            assert {c[7] for c in seen} == {1, 67} and {(c[2], c[3]) for c in seen} == {(e, j) for e in (1, 2, 16) for j in range(e)}
    key = prng.prng_key(2024)
    for scheme, name, E_, j, L_, l, D, B, rate in cases:
        layout = tw.LAYOUTS[name](B)
        got = ctx.droq_mask(key, layout, j, E_, l, L_, B, D, rate, scheme).cpu().numpy()
        exp = tw.mask_stream(key, layout, j, E_, l, L_, B, D, rate, bool(scheme))
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), exp), (scheme, name, E_, j, L_, l, D, B, rate)
    # rate 0 keeps everything
    assert ctx.droq_mask(key, tw.LAYOUTS["online"](5), 0, 2, 0, 2, 5, 64, 0.0).all()


@pytest.mark.parametrize("what,code,word", [("rate_one", -1, "rate"), ("d_832", -4, "multiple of 64"), ("d_100", -4, "multiple of 64"),
                                            ("j_is_e", -1, "0 <= j < E"), ("row_past_count", -1, "below count")])
def test_entry_points_refuse_and_write_nothing(ctx, dev, what, code, word):
    from rlx_amd.hip import RlxError
    D, rate, j, layout = 64, 0.25, 0, (3, 3, 3 * 4 + 2)
    if what == "rate_one":
        rate = 1.0
    elif what == "d_832":
        D = 832
    elif what == "d_100":
        D = 100
    elif what == "j_is_e":
        j = 2
    elif what == "row_past_count":
        layout = (3, 3, 11)                                                          # row 3's key would be keys[12] of 11
    Z, H, gb = torch.zeros(4, D, device=dev), torch.zeros(4, D, device=dev), torch.zeros(2 * D, device=dev)
    for call in (lambda: ctx.droq_block(Z, H, gb, prng.prng_key(1), layout, j, 2, 0, 2, rate),
                 lambda: ctx.droq_mask(prng.prng_key(1), layout, j, 2, 0, 2, 4, D, rate)):
        with pytest.raises(RlxError) as e:
            call()
        assert f"rc={code}" in str(e.value) and word in str(e.value), str(e.value)
    assert torch.count_nonzero(H).item() == 0


if __name__ == "__main__":      # SEEDS and the float32 gaps behind F32_GAP (CPU only)
    seeds, gaps = {}, {}
    for D in DS:
        for rate in RATES:
            gaps[(D, rate)] = {}
            for M in MS:
                seed = next(s for s in range(1000) if case_is_usable(make_case(D, M, rate, s), D, rate))
                seeds[(D, M, rate)] = seed
                c = make_case(D, M, rate, seed)
                exp, _ = twin_block(c, D, rate)
                got, _ = twin_block(c, D, rate, np.float32)
                gaps[(D, rate)][M] = tuple(float(f"{_rel(got[k], exp[k]):.2e}") for k in OUTS)
    print("SEEDS = {" + ", ".join(f"{k}: {v}" for k, v in seeds.items()) + "}")
    print("F32_GAP = {")
    for k, v in gaps.items():
        print(f"    {k}: {v},")
    print("}")
