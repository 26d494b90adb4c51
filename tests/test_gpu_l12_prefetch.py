"""GPU: the prefetching form of the fused first + second layer forward (option l12_prefetch = 1: k_l12fwd_pf takes the first-layer
weight fragments of a row tile's z1 product from registers -- the previous tile's layer-2 K loop wraps its last two refills into the
first-layer image and requests the rest behind its last product, a workgroup's first tile requests all eight at the top of the
kernel -- requests the next tile's observations behind them without a branch and stages them behind the K loop) against the form
it replaces (= 0: k_l12fwd, fragments and observations loaded at the tile top).

Every accumulator sees the same MFMAs in the same order on the same operand words and the stores are the same -- only the instant at
which an operand is requested moves -- so whole updates must come out BIT-IDENTICAL: torch.equal on both parameter vectors, all four
Adam moments and the metric rows.  That the new entry really ran is read from the library's counter l12fwd_pf_launches (the profiler
books both forms under the same row): with the option at 1 it rises by exactly the number of k_l12fwd launches of the update, with 0
by none.

Cases: one per way the moved loads can go wrong.  The kernel's grid is min(tiles, 2 x CUs), or min(tiles, CUs) per network in a twin
launch, so the row counts that put one, two or three tiles on a workgroup come from the device's CU count: one tile (prologue requests
only, nothing wraps; plain stores), two (both observation buffers, one wrap; nontemporal stores), three for some workgroups (the
buffer parity returns, a second wrap), a ragged last tile, the twin launch with one and with two tiles per workgroup (blockIdx.y == 1
must wrap into ITS first-layer image), an observation width of 12 (one 16-k block in use: the second is fetched and not multiplied)
and of 32 (both full), observations x 1e4 (the xmax scale sits behind the moved loads), all-zero rows, the data-parallel entry,
dw_recompute = 1 (no h1 store), and the settings under which the new form is not selected and the option must change nothing.

Helpers after tests/test_gpu_l1_wrap_refill.py, with the second hidden width as a parameter."""
import numpy as np
import pytest
import torch

from oracle import nets
from rlx_amd.hip import Ctx, PpoHparams, mlp_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

A = 6
OPT = "l12_prefetch"
COUNTER = "l12fwd_pf_launches"


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _nets(dev, seed, O, zero_b1=False, h2=256):
    rng = np.random.default_rng(seed)
    if h2 == 256:
        ps, cs = nets.make_spec("B", O, A, True), nets.make_spec("B", O, 1, False)
        assert list(ps.hidden) == [512, 256, 128] and list(cs.hidden) == [512, 256, 128]
    else:
        ps = nets.MLPSpec(O, [512, h2, 128], A, nets.ACT_ELU, True, True)
        cs = nets.MLPSpec(O, [512, h2, 128], 1, nets.ACT_ELU, True, False)
    pp = (nets.init_params(ps, rng, 0.01) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    cp = (nets.init_params(cs, rng, 1.0) + 0.02 * rng.standard_normal(cs.n_params)).astype(np.float32)
    if zero_b1:      # with an all-zero observation row: z1 == 0 exactly, variance 0, 1 / std = 1000
        for spec, p in ((ps, pp), (cs, cp)):
            p[spec.layers[0]["b"]:spec.layers[0]["b"] + 512] = 0.0
    pd = mlp_desc(O, ps.hidden, A, ps.act, True, True)
    cd = mlp_desc(O, cs.hidden, 1, cs.act, True, False)
    return ps, cs, pd, cd, torch.from_numpy(pp).to(dev), torch.from_numpy(cp).to(dev)


def _rollout(dev, T, N, seed, O, data=None):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    S, Ac, LP, R, AD = r(T, N, O), r(T, N, A), 0.1 * r(T, N) - 8.5, r(T, N), 2 * r(T, N) + 0.5
    rows = S.view(-1, O)
    if data == "x1e4":
        S *= 1e4
    elif data == "zero32":           # 32 all-zero rows that straddle two of the rollout's 32-row tiles (with a zero first-layer bias: _nets)
        rows[2064:2096] = 0.0
    else:
        assert data is None
    return S, Ac, LP, R, AD


def _launches(rows):
    """k_l12fwd launches of the profiled call, whatever their shape row"""
    return sum(r["launches"] for r in rows if r["kernel"] == "k_l12fwd")


def _update(dev, pf, T, N, E, MB, O=17, twin=-1, data=None, opts=(), seed=11, h2=256):
    """One rlx_ppo_update_f32 call from the seeded initial state -> (P, C, pm, pv, cm, cv, metrics), k_l12fwd launches, the
    counter's rise over the call, initial nets."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, seed, O, zero_b1=data in ("zero32",), h2=h2)
    roll = _rollout(dev, T, N, seed, O, data)
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = E * (T * N // MB)
    lr = np.linspace(4e-4, 3e-4, n_upd).astype(np.float32)
    c = Ctx(0)
    try:
        c.set_option("ppo_twin", twin)
        for k, v in opts:
            c.set_option(k, v)
        c.set_option(OPT, pf)
        P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
        pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
        n0 = c.get_counter(COUNTER)
        c.prof_begin()
        _, cnt = c.ppo_update(pd, P, pm, pv, cd, C, cm, cv, *roll, E, MB, L.prng_key(3), 0, lr, hp, met)
        torch.cuda.synchronize()
        c.prof_end()
        launches = _launches(c.prof_rows())
        rose = c.get_counter(COUNTER) - n0
        assert cnt == n_upd
    finally:
        c.close()
    return (P, C, pm, pv, cm, cv, met), launches, rose, (P0, C0)


def _assert_identical(a, b):
    for name, x, y in zip(("policy", "critic", "policy m", "policy v", "critic m", "critic v", "metrics"), a, b):
        assert torch.isfinite(y).all(), name
        assert torch.equal(x, y), (name, (x - y).abs().max().item())


def _assert_trained(a, P0, C0):
    assert (a[0] - P0).abs().max().item() > 1e-4 and (a[1] - C0).abs().max().item() > 1e-4


def _both(dev, T, N, E, MB, per_update, active=True, **kw):
    """The update with l12_prefetch = 0 and = 1: equal bit for bit, it trained, k_l12fwd ran `per_update` times per update in both
    runs (where it runs at all: per_update None skips that); active: with = 1 every one of those launches was the new entry (the
    counter), with = 0 none; not active: the counter stays where it was in both runs."""
    a, l0, c0, (P0, C0) = _update(dev, 0, T, N, E, MB, **kw)
    b, l1, c1, _ = _update(dev, 1, T, N, E, MB, **kw)
    n_upd = E * (T * N // MB)
    print(f"k_l12fwd launches {l0} / {l1}, {COUNTER} rose by {c0} / {c1}")
    if per_update is not None:
        assert l0 == per_update * n_upd and l1 == per_update * n_upd, (l0, l1)
    assert c0 == 0, c0
    assert c1 == (l1 if active else 0), (c1, l1)
    _assert_identical(a, b)
    _assert_trained(a, P0, C0)


def test_option_takes_zero_or_one_only(dev):
    c = Ctx(0)
    try:
        for bad in (2, -1, 8):
            with pytest.raises(Exception):
                c.set_option(OPT, bad)
        c.set_option(OPT, 0)
        c.set_option(OPT, 1)
        assert c.get_counter(COUNTER) == 0
    finally:
        c.close()


def test_one_tile_per_workgroup(dev):
    """4096-row minibatches: 128 tiles on 128 workgroups per network, two streams, the plain-store entry -- every tile takes the
    fragments the prologue requested, the wrapped refills fetch for nothing; 4 updates."""
    _both(dev, 2, 4096, 2, 4096, per_update=2)


def test_two_tiles_per_workgroup_nontemporal(dev):
    """one update at 4 x 32 x (compute units) rows (32768 on 256) without the twin launch: two tiles on each of the 2 x CUs
    workgroups, the nontemporal entry -- both observation buffers, and the second tile's z1 from the first tile's wrapped refills."""
    mb = 32 * 4 * _cus(dev)
    assert mb >= 16384
    _both(dev, 1, mb, 1, mb, per_update=2, twin=0)


def test_three_tiles_for_some_workgroups(dev):
    """one more tile than two per workgroup (32768 + 32 rows on 256 CUs): workgroup 0 runs three -- the buffer parity returns to 0, a
    second wrap -- beside workgroups that run two."""
    mb = 32 * 4 * _cus(dev) + 32
    _both(dev, 1, mb, 1, mb, per_update=2, twin=0)


def test_ragged_last_tile(dev):
    """4100 rows are 128 tiles and 4 rows (no multiple of 64 either: the plain head / trunk path): rows past M are loaded as
    zeros by lanes that keep their load; 2 updates."""
    _both(dev, 2, 2050, 2, 4100, per_update=2)


@pytest.mark.parametrize("tiles", [1, 2])
def test_twin_launch(dev, tiles):
    """ppo_twin = 1 at tiles x 32 x (compute units) rows (8192, 16384 on 256): grid.y == 2 with CUs workgroups per network,
    blockIdx.y == 1 is the critic and must wrap into ITS first-layer image; one and two tiles per workgroup; 2 updates."""
    mb = 32 * tiles * _cus(dev)
    _both(dev, 2, mb, 1, mb, per_update=1, twin=1)


@pytest.mark.parametrize("O", [12, 32])
def test_observation_width(dev, O):
    """12 observations: one 16-k block of the first-layer image in use -- the second (all zero words, it exists in the image) is
    fetched and never multiplied.  32: both blocks full, every fragment word of both in use.  4096 rows, 2 updates."""
    _both(dev, 1, 8192, 1, 4096, per_update=2, O=O)


@pytest.mark.parametrize("data", ["x1e4", "zero32"])
def test_data_edges(dev, data):
    """4096 rows, 4 updates each.  x1e4: the observation planes' scale comes from the pass's max |x| and sits behind the moved
    loads.  zero32: 32 all-zero rows straddling two tiles with a zero first-layer bias -- z1 == 0 from the register-held fragments,
    variance exactly 0, the clamp decides."""
    _both(dev, 2, 2048, 4, 4096, per_update=2, data=data)


def test_dw_recompute_stores_statistics_only(dev):
    """dw_recompute = 1: no h1 store in the normalise phase, the statistics array only; 4096 rows, 4 updates."""
    _both(dev, 2, 4096, 2, 4096, per_update=2, opts=(("dw_recompute", 1),))


@pytest.mark.parametrize("opts,h2", [((("ln_row_once", 0),), 256), ((("gemm_bx", 0),), 256), ((("l12_fused", 0),), 256), ((), 512)],
                         ids=["ln_row_once0", "gemm_bx0", "l12_fused0", "hidden1_512"])
def test_inactive_where_the_new_form_is_not_selected(dev, opts, h2):
    """ln_row_once = 0 (the earlier statistics form), gemm_bx = 0 or l12_fused = 0 (k_l12fwd does not run) and hidden[1] = 512 (two
    column tiles per wave in layer 2): l12_prefetch = 1 changes nothing -- the counter stays, the results are equal bit for bit, the
    update trains."""
    per = 2 if (opts and opts[0][0] == "ln_row_once") or h2 == 512 else None
    _both(dev, 2, 4096, 1, 4096, per_update=per, active=False, opts=opts, h2=h2)


class _Buf:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _dist_update(dev, pf, T, NG, nl, world, MB, seed=5, O=17):
    """Rank 0 of `world` emulated ranks through rlx_ppo_update_dist_f32 (the hook leaves every buffer as it is: the local
    contribution alone) -> results, the valid-row counts the hook saw, k_l12fwd launches, the counter's rise."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, seed, O)
    mine = tuple(x[:, :nl].contiguous() for x in _rollout(dev, T, NG, seed, O))
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = T * NG // MB
    me = Ctx(0)
    seen = {}
    try:
        me.set_rank(0, world)
        me.set_option(OPT, pf)
        assert me.dist_row_capacity(MB, nl, NG) == 4608

        def hook(ptr, n, dtype, on_side):
            if dtype == 1:
                torch.cuda.current_stream().synchronize()
                seen["stats"] = torch.as_tensor(_Buf(ptr, n, "<f8"), device=dev).clone().view(n_upd, 4)
        me.set_allreduce_hook(hook)
        P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
        pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
        n0 = me.get_counter(COUNTER)
        me.prof_begin()
        me.ppo_update_dist(pd, P, pm, pv, cd, C, cm, cv, *mine, NG, 0, 1, MB, L.prng_key(3), 0, np.full(n_upd, 4e-4, np.float32), hp, met)
        torch.cuda.synchronize()
        me.prof_end()
        launches = _launches(me.prof_rows())
        rose = me.get_counter(COUNTER) - n0
        me.set_allreduce_hook(None)
    finally:
        me.close()
    return (P, C, pm, pv, cm, cv, met), seen, launches, rose, (P0, C0)


def test_data_parallel_entry_on_one_rank(dev):
    """Data-parallel entry, rank 0 of 8: global minibatches of 32768 rows, 512 of 4096 envs local -> a per-rank capacity of 4608
    rows (144 tiles) of which about 4096 are valid and ragged: the rows past the valid count are all-zero rows inside M."""
    T, NG, nl, world, MB = 16, 4096, 512, 8, 32768
    a, seen, l0, c0, (P0, C0) = _dist_update(dev, 0, T, NG, nl, world, MB)
    b, _, l1, c1, _ = _dist_update(dev, 1, T, NG, nl, world, MB)
    counts = seen["stats"][:, 2].cpu()
    assert all(0 < int(c) < 4608 for c in counts) and len(set(int(c) for c in counts)) > 1        # fewer valid rows than capacity, ragged
    print(f"k_l12fwd launches {l0} / {l1}, {COUNTER} rose by {c0} / {c1}")
    assert l0 == l1 and l1 > 0, (l0, l1)
    assert c0 == 0 and c1 == l1, (c0, c1, l1)
    _assert_identical(a, b)
    _assert_trained(a, P0, C0)
