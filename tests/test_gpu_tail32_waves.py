"""GPU: k_tail32_bx on eight waves per 32-row tile (option tail32_waves = 8) against the four-wave form (= 4).

The eight-wave form keeps the tile, the LDS layout and every sum's operands and order, so whole updates must come out
BIT-IDENTICAL (torch.equal on parameters, Adam moments and metric rows after several Adam steps): through the single launches
of the two-chain schedule at the edges of the head's 8-wide action padding, through the twin launch (grid.y = 2) and through
the data-parallel entry with rows past the valid count.  Against other kernels (the three launches the tail replaces) it is
held to the bars tests/test_gpu_twin_update.py sets between different kernels.

Nets: 512-LN-256-128 ELU on 17 observations (the kernel is specialised to a 256-wide layer below a 128-wide last one); 4096 rows
is the smallest minibatch the tail takes."""
import numpy as np
import pytest
import torch

from oracle import nets
from oracle.sharding import local_minibatches
from rlx_amd.hip import Ctx, PpoHparams, mlp_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

O = 17


def _nets(dev, A, seed):
    rng = np.random.default_rng(seed)
    ps, cs = nets.make_spec("B", O, A, True), nets.make_spec("B", O, 1, False)
    assert list(ps.hidden) == [512, 256, 128] and list(cs.hidden) == [512, 256, 128]
    pp = (nets.init_params(ps, rng, 0.01) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    cp = (nets.init_params(cs, rng, 1.0) + 0.02 * rng.standard_normal(cs.n_params)).astype(np.float32)
    pd = mlp_desc(O, ps.hidden, A, ps.act, True, True)
    cd = mlp_desc(O, cs.hidden, 1, cs.act, True, False)
    return ps, cs, pd, cd, torch.from_numpy(pp).to(dev), torch.from_numpy(cp).to(dev)


def _rollout(dev, T, N, A, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    return r(T, N, O), r(T, N, A), 0.1 * r(T, N) - 8.5, r(T, N), 2 * r(T, N) + 0.5


def _update(dev, waves, T, N, E, MB, A=6, twin=-1, tail=2, seed=11, prof=False):
    """One rlx_ppo_update_f32 call from the seeded initial state -> (P, C, pm, pv, cm, cv, metrics), profile rows."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, A, seed)
    roll = _rollout(dev, T, N, A, seed)
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = E * (T * N // MB)
    lr = np.linspace(4e-4, 3e-4, n_upd).astype(np.float32)
    c = Ctx(0)
    try:
        c.set_option("ppo_twin", twin)
        c.set_option("ppo_tail", tail)
        if waves:
            c.set_option("tail32_waves", waves)
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


def _tail_launches(rows, MB):
    return {(r["kernel"], r["engine"], r["M"], r["N"], r["K"]): r["launches"] for r in rows}.get(("k_tail", 1, MB, 128, 256))


def _assert_identical(a, b):
    for name, x, y in zip(("policy", "critic", "policy m", "policy v", "critic m", "critic v", "metrics"), a, b):
        assert torch.isfinite(y).all(), name
        assert torch.equal(x, y), (name, (x - y).abs().max().item())


@pytest.mark.parametrize("A", [1, 6, 8])      # 8: the kernel's limit; 1 and 8: the edges of the head's 8-wide padding
def test_eight_wave_update_is_bit_identical_to_the_four_wave_update(dev, A):
    T, N, E, MB = 2, 4096, 2, 4096            # 4 updates: a difference in any gradient bit would compound through Adam
    a, rows, (P0, C0) = _update(dev, 4, T, N, E, MB, A=A, prof=True)
    b, _, _ = _update(dev, 8, T, N, E, MB, A=A)
    assert _tail_launches(rows, MB) == 2 * E * (T * N // MB)          # the tail ran, one launch per network and update
    _assert_identical(a, b)
    assert (a[0] - P0).abs().max().item() > 1e-4 and (a[1] - C0).abs().max().item() > 1e-4      # it trained


def test_option_takes_four_or_eight_only(dev):
    c = Ctx(0)
    try:
        for bad in (0, 2, 6, 16, -1):
            with pytest.raises(Exception):
                c.set_option("tail32_waves", bad)
        c.set_option("tail32_waves", 8)
        c.set_option("tail32_waves", 4)
    finally:
        c.close()


def test_twin_launch_is_bit_identical(dev):
    """grid.y == 2: blockIdx.y == 1 is the critic's body in the same launch."""
    T, N, E, MB = 2, 8192, 2, 8192
    a, rows, _ = _update(dev, 4, T, N, E, MB, twin=1, tail=2, prof=True)
    b, _, _ = _update(dev, 8, T, N, E, MB, twin=1, tail=2)
    assert _tail_launches(rows, MB) == E * (T * N // MB)              # ONE launch per update covers both networks
    _assert_identical(a, b)


def _dist_update(dev, waves, T, NG, nl, world, MB, seed=5):
    """Rank 0 of `world` emulated ranks through rlx_ppo_update_dist_f32 (the hook leaves every buffer as it is: the local
    contribution alone).  -> results, the local gradients and advantage sums the hook saw, what the reference needs."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, 6, seed)
    S, Ac, LP, R, AD = _rollout(dev, T, NG, 6, seed)
    mine = tuple(x[:, :nl].contiguous() for x in (S, Ac, LP, R, AD))
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = T * NG // MB
    key = L.prng_key(3)
    me = Ctx(0)
    seen = {}
    try:
        me.set_rank(0, world)
        me.set_option("tail32_waves", waves)
        assert me.dist_row_capacity(MB, nl, NG) == 4608

        def hook(ptr, n, dtype, on_side):
            if dtype == 1:
                torch.cuda.current_stream().synchronize()
                seen["stats"] = torch.as_tensor(_Buf(ptr, n, "<f8"), device=dev).clone().view(n_upd, 4)
            elif n != n_upd * 10:
                st = me_side if on_side else torch.cuda.current_stream()
                with torch.cuda.stream(st):
                    seen.setdefault("c" if on_side else "p", []).append(torch.as_tensor(_Buf(ptr, n, "<f4"), device=dev).clone())
        me_side = me.side_stream()
        me.set_allreduce_hook(hook)
        P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
        pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
        me.ppo_update_dist(pd, P, pm, pv, cd, C, cm, cv, *mine, NG, 0, 1, MB, key, 0, np.full(n_upd, 4e-4, np.float32), hp, met)
        torch.cuda.synchronize()
        me.set_allreduce_hook(None)
    finally:
        me.close()
    return (P, C, pm, pv, cm, cv, met), seen, (ps, cs, pd, cd, P0, C0, mine, hp, key)


class _Buf:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def test_rows_past_the_valid_count(ctx, dev):
    """Data-parallel entry, rank 0 of 8: global minibatches of 32768 rows, 512 of 4096 envs local -> a per-rank capacity of 4608
    rows of which about 4096 are valid (ragged: two minibatches per epoch).  Both forms agree bit for bit, and the zero-weight rows
    leave the gradients what a pass over exactly the valid rows gives (the per-phase entry on the compacted rows, at the bar of
    tests/test_gpu_sharded_update.py: 1e-5 of the gradient's norm)."""
    T, NG, nl, world, MB = 16, 4096, 512, 8, 32768
    a, _, _ = _dist_update(dev, 4, T, NG, nl, world, MB)
    b, seen, (ps, cs, pd, cd, P0, C0, mine, hp, key) = _dist_update(dev, 8, T, NG, nl, world, MB)
    _assert_identical(a, b)
    n_upd = T * NG // MB
    perm = torch.empty(T * NG, dtype=torch.int32, device=dev)
    ctx.permutation(key, perm, 1, T * NG)
    compact, counts, offsets = local_minibatches(perm.cpu(), n_upd, MB, NG, nl, 0)
    assert all(0 < int(c) < 4608 for c in counts) and len(set(int(c) for c in counts)) > 1        # fewer valid rows than capacity, ragged
    assert torch.equal(seen["stats"][:, 2].cpu(), counts.double())
    # first update: parameters are still the initial ones
    idx = compact[offsets[0]:offsets[1]].to(dev)
    g_p, g_c, m = torch.zeros(ps.n_params, device=dev), torch.zeros(cs.n_params, device=dev), torch.zeros(8, device=dev)
    ctx.ppo_minibatch_fwd_bwd(pd, P0, g_p, cd, C0, g_c, m, *mine, idx, hp, mb_global=MB, stats_io=seen["stats"][0].clone(), phase=2)
    torch.cuda.synchronize()
    for got, exp in ((seen["p"][0], g_p), (seen["c"][0], g_c)):
        got, exp = got.cpu().numpy(), exp.cpu().numpy()
        assert np.all(np.isfinite(got))
        assert np.linalg.norm(got - exp) / np.linalg.norm(exp) < 1e-5


def test_eight_wave_tail_matches_the_three_launch_update(dev):
    """tail32_waves = 8 against ppo_tail = 0 (k_gemm_bx<0>, k_head_loss_fast, k_gemm_bx<1>) at 4096 rows, at the bars of
    test_gpu_twin_update.py::test_tail_kernel_update_matches_the_three_launch_update for the 32-row form."""
    T, N, E, MB = 16, 1024, 2, 4096
    a, _, _ = _update(dev, 0, T, N, E, MB, twin=0, tail=0)
    b, rows, _ = _update(dev, 8, T, N, E, MB, twin=0, tail=2, prof=True)
    n_upd = E * (T * N // MB)
    ma, mb_ = a[6].cpu().numpy(), b[6].cpu().numpy()
    assert np.all(np.isfinite(mb_))
    np.testing.assert_allclose(mb_[0, [0, 1, 2, 3, 5, 6, 7, 8, 9]], ma[0, [0, 1, 2, 3, 5, 6, 7, 8, 9]], rtol=5e-6, atol=1e-7)
    np.testing.assert_allclose(mb_[0, 4], ma[0, 4], rtol=0, atol=1.5 / MB)
    np.testing.assert_allclose(mb_[:, [0, 1, 3, 8, 9]], ma[:, [0, 1, 3, 8, 9]], rtol=2e-3, atol=2e-5)
    for x, y in ((a[0], b[0]), (a[1], b[1])):
        d = (x - y).abs().cpu().numpy()
        ref = x.abs().cpu().numpy()
        assert (d <= 2e-5 + 1e-3 * ref).mean() > 0.995, (d.max(), (d > 2e-5).mean())
    ran = {(r["kernel"], r["engine"], r["M"], r["N"], r["K"]): r["launches"] for r in rows}
    assert ran.get(("k_tail", 1, MB, 128, 256)) == 2 * n_upd, ran
    assert ("k_gemm_fwd", 1, MB, 128, 256) not in ran and ("k_gemm_dx", 1, MB, 256, 128) not in ran
