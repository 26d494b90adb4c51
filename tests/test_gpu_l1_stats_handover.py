"""GPU: the LayerNorm row statistics handed from k_l12fwd to the fused first-layer backward of the same minibatch pass (option
l1_stats_handover = 1: k_l12fwd leaves mean | 1 / std per row in a [2][M] array next to h1, k_dx_l1bwd_stats loads them) against
the earlier kernels (= 0: k_dx_l1bwd<ROW1> rebuilds them from its recomputed z1 -- partial sums, LDS partials, a workgroup barrier,
the fold, ln_row_stats).

Both kernels form z1 with the same product and the statistics with the same code, so the loaded words are the words the backward
would compute and whole updates must come out BIT-IDENTICAL: torch.equal on both parameter vectors, all four Adam moments and the
metric rows after several Adam steps -- a difference in any gradient bit would compound through Adam.  One case per instantiation
the option selects (single, twin and nontemporal-forward launches, dw_recompute = 1 where one array serves both readers, the
data-parallel entry with rows past the valid count, a minibatch that is no multiple of the 32-row tile) and one per data condition
that moves 1 / std to an edge: observations of another magnitude (the dW1 operand's scale takes the first tile's largest 1 / std,
now from the loaded values), rows whose variance is zero or rounds to just below it (the clamp), all-zero observation rows.

That the handover form really ran is read from the profiler rows: its launches are booked under the same row as k_dx_l1bwd, with 8
more bytes per row and network (the two loaded statistics), and k_l12fwd's row grows by the same 8 bytes it now writes.

Nets: 512-LN-256-128 ELU on 17 observations, as tests/test_gpu_ln_row_once.py (whose helpers are copied here).  The minibatch gather
permutes the rollout's rows, so the marked rows land in tiles of their own choosing; the conditions are per row and hold wherever a
row lands."""
import numpy as np
import pytest
import torch

from oracle import nets
from rlx_amd.hip import Ctx, PpoHparams, mlp_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

O, A = 17, 6
OPT = "l1_stats_handover"


def _nets(dev, seed, zero_b1=False):
    rng = np.random.default_rng(seed)
    ps, cs = nets.make_spec("B", O, A, True), nets.make_spec("B", O, 1, False)
    assert list(ps.hidden) == [512, 256, 128] and list(cs.hidden) == [512, 256, 128]
    pp = (nets.init_params(ps, rng, 0.01) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    cp = (nets.init_params(cs, rng, 1.0) + 0.02 * rng.standard_normal(cs.n_params)).astype(np.float32)
    if zero_b1:      # with an all-zero observation row: z1 == 0 exactly, variance 0, 1 / std = 1000
        for spec, p in ((ps, pp), (cs, cp)):
            p[spec.layers[0]["b"]:spec.layers[0]["b"] + 512] = 0.0
    pd = mlp_desc(O, ps.hidden, A, ps.act, True, True)
    cd = mlp_desc(O, cs.hidden, 1, cs.act, True, False)
    return ps, cs, pd, cd, torch.from_numpy(pp).to(dev), torch.from_numpy(cp).to(dev)


def _rollout(dev, T, N, seed, data=None):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    S, Ac, LP, R, AD = r(T, N, O), r(T, N, A), 0.1 * r(T, N) - 8.5, r(T, N), 2 * r(T, N) + 0.5
    rows = S.view(-1, O)
    if data == "x1e4":
        S *= 1e4
    elif data == "x1e-3":
        S *= 1e-3
    elif data == "identical64":      # 64 equal observation rows: equal statistics, whatever tiles they land in
        rows[1000:1064] = rows[1000].clone()
    elif data == "constant64":       # 64 rows whose z1 is the same in every column: sum z^2 / 512 - mean^2 rounds to 0 or just below
        rows[1000:1064] = 0.0
    elif data == "zero32":           # 32 all-zero rows that straddle two of the rollout's 32-row tiles (with a zero first-layer bias: _nets)
        rows[2064:2096] = 0.0
    else:
        assert data is None
    return S, Ac, LP, R, AD


def _update(dev, hand, T, N, E, MB, twin=-1, data=None, opts=(), seed=11, prof=False):
    """One rlx_ppo_update_f32 call from the seeded initial state -> (P, C, pm, pv, cm, cv, metrics), profile rows, initial nets."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, seed, zero_b1=data in ("zero32",))
    if data == "constant64":         # first-layer bias the same in every column: an all-zero observation row has z1 = 0.3 everywhere
        for spec, p in ((ps, P0), (cs, C0)):
            p[spec.layers[0]["b"]:spec.layers[0]["b"] + 512] = 0.3
    roll = _rollout(dev, T, N, seed, data)
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = E * (T * N // MB)
    lr = np.linspace(4e-4, 3e-4, n_upd).astype(np.float32)
    c = Ctx(0)
    try:
        c.set_option("ppo_twin", twin)
        for k, v in opts:
            c.set_option(k, v)
        c.set_option(OPT, hand)
        P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
        pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
        if prof:
            c.prof_begin()
        _, cnt = c.ppo_update(pd, P, pm, pv, cd, C, cm, cv, *roll, E, MB, L.prng_key(3), 0, lr, hp, met)
        torch.cuda.synchronize()
        rows = None
        if prof:
            c.prof_end()
            rows = c.prof_rows()
        assert cnt == n_upd
    finally:
        c.close()
    return (P, C, pm, pv, cm, cv, met), rows, (P0, C0)


def _row(rows, kernel, MB):
    """(launches, bytes) of the kernel's profiler row on the split-operand engine at MB rows; every launch is timed (prof_sample 1)"""
    key = {"k_l12fwd": (MB, 256, 512), "k_dx_l1bwd": (MB, 512, 256)}[kernel]
    got = [r for r in rows if r["kernel"] == kernel and r["engine"] == 1 and (r["M"], r["N"], r["K"]) == key]
    assert len(got) == 1, (kernel, rows)
    assert got[0]["timed"] == got[0]["launches"]
    return got[0]["launches"], got[0]["bytes"]


def _assert_identical(a, b):
    for name, x, y in zip(("policy", "critic", "policy m", "policy v", "critic m", "critic v", "metrics"), a, b):
        assert torch.isfinite(y).all(), name
        assert torch.equal(x, y), (name, (x - y).abs().max().item())


def _assert_trained(a, P0, C0):
    assert (a[0] - P0).abs().max().item() > 1e-4 and (a[1] - C0).abs().max().item() > 1e-4


def _both(dev, T, N, E, MB, per_update, active=True, fwd_grows=True, **kw):
    """The update with l1_stats_handover = 0 and = 1: equal bit for bit, both kernels ran `per_update` times per update in both runs,
    it trained.  active: the handover form must have run with = 1 (its row carries the statistics' 8 bytes per row and network;
    fwd_grows: k_l12fwd's row grows by the same bytes -- not under dw_recompute, where it writes the array in both runs); not active:
    the option must change nothing, the rows' bytes included."""
    a, rows0, (P0, C0) = _update(dev, 0, T, N, E, MB, prof=True, **kw)
    b, rows1, _ = _update(dev, 1, T, N, E, MB, prof=True, **kw)
    n_upd = E * (T * N // MB)
    nets_per_launch = 2 // per_update
    extra = 8.0 * MB * nets_per_launch * per_update * n_upd
    for kernel, grows in (("k_l12fwd", active and fwd_grows), ("k_dx_l1bwd", active)):
        (l0, b0), (l1, b1) = _row(rows0, kernel, MB), _row(rows1, kernel, MB)
        assert l0 == per_update * n_upd and l1 == per_update * n_upd, (kernel, l0, l1)
        assert b1 - b0 == (extra if grows else 0.0), (kernel, b0, b1, extra)
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
    finally:
        c.close()


def test_two_chain_updates_are_bit_identical(dev):
    """4096-row minibatches: single launches per network on two streams (the plain-store k_l12fwd, k_dx_l1bwd_stats<TWIN = false>),
    each network with the statistics slot of its own scratch bank; 4 updates."""
    _both(dev, 2, 4096, 2, 4096, per_update=2)


def test_twin_launch_is_bit_identical(dev):
    """8192-row minibatches: grid.y == 2, blockIdx.y == 1 is the critic with its own statistics array in the same launch; 4 updates."""
    _both(dev, 2, 8192, 2, 8192, per_update=1, twin=1)


def test_nontemporal_forward_is_bit_identical(dev):
    """one update at 16384 rows without the twin launch: the k_l12fwd instantiation that stores h1 past the L2 writes the array too."""
    _both(dev, 2, 8192, 1, 16384, per_update=2, twin=0)


def test_dw_recompute_shares_the_statistics_array(dev):
    """dw_recompute = 1: k_l12fwd stores the statistics WITHOUT h1 (in both runs), and with the handover the layer-2 weight gradient
    and the fused first-layer backward both read that one array."""
    _both(dev, 2, 4096, 2, 4096, per_update=2, fwd_grows=False, opts=(("dw_recompute", 1),))


@pytest.mark.parametrize("data", ["x1e4", "x1e-3", "identical64", "constant64", "zero32"])
def test_data_conditions(dev, data):
    """4096 rows, 4 updates each.  x1e4 / x1e-3: 1 / std of every row moves by that factor, and with it the power-of-two scale of
    the dW1 operand (the first tile's largest 1 / std, now taken from the loaded values).  constant64: z1 = 0.3 in all 512 columns
    of 64 rows -- sum z^2 / 512 - mean^2 is rounding noise around 0, the clamp decides.  zero32: z1 == 0, variance exactly 0,
    1 / std = rsqrt(1e-6) = 1000."""
    _both(dev, 2, 2048, 4, 4096, per_update=2, data=data)


def test_minibatch_that_is_no_multiple_of_the_tile(dev):
    """rlx_ppo_update_f32 takes any minibatch size that divides the batch: 4100 rows are 128 tiles and 4 rows.  (No multiple of 64
    either, so the row-tile tail kernel is out and the pair runs through the plain head / trunk path.)  The forward writes the
    statistics of the 4 valid rows of the last tile; the backward gives the 28 rows past M the fixed pair 0 | 1 where the
    earlier kernels compute the statistics of z1 = b1 -- their dZ2 rows are zero, so every term they add is +-0 under any finite
    pair and no accumulator bit may change.  2 updates."""
    _both(dev, 2, 2050, 2, 4100, per_update=2)


@pytest.mark.parametrize("opts", [(("ln_row_once", 0),), (("gemm_bx", 0),)], ids=["ln_row_once0", "gemm_bx0"])
def test_inactive_where_the_pair_is_not_the_same_code(dev, opts):
    """ln_row_once = 0 (both kernels in their earlier forms) or gemm_bx = 0 (the exact-fp32 engine: no k_l12fwd, k_dx_l1bwd<BX =
    false>): l1_stats_handover = 1 changes nothing -- equal results bit for bit, and the update still runs and trains."""
    if opts[0][0] == "gemm_bx":
        a, _, (P0, C0) = _update(dev, 0, 2, 4096, 1, 4096, opts=opts)
        b, _, _ = _update(dev, 1, 2, 4096, 1, 4096, opts=opts)
        _assert_identical(a, b)
        _assert_trained(a, P0, C0)
    else:
        _both(dev, 2, 4096, 1, 4096, per_update=2, active=False, opts=opts)


class _Buf:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _dist_update(dev, hand, T, NG, nl, world, MB, seed=5):
    """Rank 0 of `world` emulated ranks through rlx_ppo_update_dist_f32 (the hook leaves every buffer as it is: the local
    contribution alone) -> results, the valid-row counts the hook saw."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, seed)
    mine = tuple(x[:, :nl].contiguous() for x in _rollout(dev, T, NG, seed))
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = T * NG // MB
    me = Ctx(0)
    seen = {}
    try:
        me.set_rank(0, world)
        me.set_option(OPT, hand)
        assert me.dist_row_capacity(MB, nl, NG) == 4608

        def hook(ptr, n, dtype, on_side):
            if dtype == 1:
                torch.cuda.current_stream().synchronize()
                seen["stats"] = torch.as_tensor(_Buf(ptr, n, "<f8"), device=dev).clone().view(n_upd, 4)
        me.set_allreduce_hook(hook)
        P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
        pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
        me.ppo_update_dist(pd, P, pm, pv, cd, C, cm, cv, *mine, NG, 0, 1, MB, L.prng_key(3), 0, np.full(n_upd, 4e-4, np.float32), hp, met)
        torch.cuda.synchronize()
        me.set_allreduce_hook(None)
    finally:
        me.close()
    return (P, C, pm, pv, cm, cv, met), seen, (P0, C0)


def test_rows_past_the_valid_count(dev):
    """Data-parallel entry, rank 0 of 8: global minibatches of 32768 rows, 512 of 4096 envs local -> a per-rank capacity of 4608
    rows (144 tiles) of which about 4096 are valid and ragged: the rows past the valid count are all-zero observation rows inside M,
    so the forward writes their statistics and the backward loads them like any other row's."""
    T, NG, nl, world, MB = 16, 4096, 512, 8, 32768
    a, seen, (P0, C0) = _dist_update(dev, 0, T, NG, nl, world, MB)
    b, _, _ = _dist_update(dev, 1, T, NG, nl, world, MB)
    counts = seen["stats"][:, 2].cpu()
    assert all(0 < int(c) < 4608 for c in counts) and len(set(int(c) for c in counts)) > 1        # fewer valid rows than capacity, ragged
    _assert_identical(a, b)
    _assert_trained(a, P0, C0)
