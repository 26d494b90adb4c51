"""GPU: the lean form of the eight-wave tail (k_tail32_bx_lean, option tail32_lean = 1, the default) against the kernel it replaces
(k_tail32_bx<ELU, 256, 8>, tail32_lean = 0).

The lean form pads the head weights in LDS, has waves 4-7 build act'(H2) once as an fp32 image in place of the H2 planes, runs the
serial sections on waves 4 / 5 with the metric sums in LDS slots of their own, and passes the head's weight-gradient partials
through LDS as 16-byte pieces.  Every sum keeps its operands and its order, so whole updates must come out BIT-IDENTICAL
(torch.equal on parameters, both Adam moments of both networks and the metric rows after several Adam steps): through the single
launches of the two-chain schedule at the edges of the head's 8-wide action padding (what the padded staging of the head weights
can get wrong), through the twin launch (grid.y = 2), through the data-parallel entry with rows past the valid count, and on a
network built so that the act'(H2) image holds both branches of ELU' and its boundary.

Helpers, nets (512-LN-256-128 ELU on 17 observations) and hyper-parameters (clip 0.1, entropy 0.01) as
tests/test_gpu_tail32_waves.py; 4096 rows is the smallest minibatch the tail takes."""
import numpy as np
import pytest
import torch

from oracle import nets
from rlx_amd.hip import Ctx, PpoHparams, mlp_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu

O = 17
NAMES = ("policy", "critic", "policy m", "policy v", "critic m", "critic v", "metrics")


def _nets(dev, A, seed, edit=None):
    rng = np.random.default_rng(seed)
    ps, cs = nets.make_spec("B", O, A, True), nets.make_spec("B", O, 1, False)
    assert list(ps.hidden) == [512, 256, 128] and list(cs.hidden) == [512, 256, 128]
    pp = (nets.init_params(ps, rng, 0.01) + 0.02 * rng.standard_normal(ps.n_params)).astype(np.float32)
    cp = (nets.init_params(cs, rng, 1.0) + 0.02 * rng.standard_normal(cs.n_params)).astype(np.float32)
    if edit:
        edit(ps, pp)
        edit(cs, cp)
    pd = mlp_desc(O, ps.hidden, A, ps.act, True, True)
    cd = mlp_desc(O, cs.hidden, 1, cs.act, True, False)
    return ps, cs, pd, cd, torch.from_numpy(pp).to(dev), torch.from_numpy(cp).to(dev)


def _rollout(dev, T, N, A, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    return r(T, N, O), r(T, N, A), 0.1 * r(T, N) - 8.5, r(T, N), 2 * r(T, N) + 0.5


def _update(dev, lean, T, N, E, MB, A=6, waves=8, twin=-1, tail=2, seed=11, prof=False, edit=None):
    """One rlx_ppo_update_f32 call from the seeded initial state -> (P, C, pm, pv, cm, cv, metrics), profile rows, (P0, C0)."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, A, seed, edit)
    roll = _rollout(dev, T, N, A, seed)
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = E * (T * N // MB)
    lr = np.linspace(4e-4, 3e-4, n_upd).astype(np.float32)
    c = Ctx(0)
    try:
        c.set_option("ppo_twin", twin)
        c.set_option("ppo_tail", tail)
        c.set_option("tail32_waves", waves)
        c.set_option("tail32_lean", lean)
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
    for name, x, y in zip(NAMES, a, b):
        assert torch.isfinite(y).all(), name
        assert torch.equal(x, y), (name, (x - y).abs().max().item())


@pytest.mark.parametrize("A", [1, 6, 8])      # 8: the kernel's limit; 1 and 8: the edges of the head's 8-wide padding
def test_lean_update_is_bit_identical(dev, A):
    T, N, E, MB = 2, 4096, 2, 4096            # 4 updates: a difference in any gradient bit would compound through Adam
    a, rows, (P0, C0) = _update(dev, 0, T, N, E, MB, A=A, prof=True)
    b, _, _ = _update(dev, 1, T, N, E, MB, A=A)
    assert _tail_launches(rows, MB) == 2 * E * (T * N // MB)          # the tail ran, one launch per network and update
    _assert_identical(a, b)
    assert (a[0] - P0).abs().max().item() > 1e-4 and (a[1] - C0).abs().max().item() > 1e-4      # it trained


def test_twin_launch_is_bit_identical(dev):
    """grid.y == 2: blockIdx.y == 1 is the critic's body in the same launch."""
    T, N, E, MB = 2, 8192, 2, 8192
    a, rows, _ = _update(dev, 0, T, N, E, MB, twin=1, tail=2, prof=True)
    b, _, _ = _update(dev, 1, T, N, E, MB, twin=1, tail=2)
    assert _tail_launches(rows, MB) == E * (T * N // MB)              # ONE launch per update covers both networks
    _assert_identical(a, b)


def _dist_update(dev, lean, T, NG, nl, world, MB, seed=5):
    """Rank 0 of `world` emulated ranks through rlx_ppo_update_dist_f32 (the hook leaves every buffer as it is: the local
    contribution alone)."""
    ps, cs, pd, cd, P0, C0 = _nets(dev, 6, seed)
    mine = tuple(x[:, :nl].contiguous() for x in _rollout(dev, T, NG, 6, seed))
    hp = PpoHparams(0.1, 0.01, 1.0, 5.0, 0.9, 0.999, 1e-8)
    n_upd = T * NG // MB
    me = Ctx(0)
    try:
        me.set_rank(0, world)
        me.set_option("tail32_waves", 8)
        me.set_option("tail32_lean", lean)
        assert me.dist_row_capacity(MB, nl, NG) == 4608
        me.set_allreduce_hook(lambda ptr, n, dtype, on_side: None)
        P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
        pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
        me.ppo_update_dist(pd, P, pm, pv, cd, C, cm, cv, *mine, NG, 0, 1, MB, L.prng_key(3), 0, np.full(n_upd, 4e-4, np.float32), hp, met)
        torch.cuda.synchronize()
        me.set_allreduce_hook(None)
    finally:
        me.close()
    return (P, C, pm, pv, cm, cv, met), (P0, C0)


def test_rows_past_the_valid_count(dev):
    """Data-parallel entry, rank 0 of 8, at the shapes of tests/test_gpu_tail32_waves.py::test_rows_past_the_valid_count: global
    minibatches of 32768 rows, 512 of 4096 envs local -> a per-rank capacity of 4608 rows of which about 4096 are valid."""
    T, NG, nl, world, MB = 16, 4096, 512, 8, 32768
    a, (P0, C0) = _dist_update(dev, 0, T, NG, nl, world, MB)
    b, _ = _dist_update(dev, 1, T, NG, nl, world, MB)
    _assert_identical(a, b)
    assert (a[0] - P0).abs().max().item() > 1e-4 and (a[1] - C0).abs().max().item() > 1e-4


def _act_edge(spec, p):
    """Second layer: columns 0-31 with zero weights and bias -- h2 = ELU(0) = 0 exactly, the boundary of ELU' (h2 > 0 ? 1 : h2 + 1);
    columns 32-63 with zero weights and a bias of -20 -- h2 = ELU(-20) ~ -1, the other branch at its far end (h2 + 1 ~ 0); the
    rest random (both branches, mixed)."""
    l2 = spec.layers[1]
    assert (l2["in"], l2["out"]) == (512, 256)
    w = p[l2["W"]:l2["W"] + 512 * 256].reshape(512, 256)
    w[:, :64] = 0.0
    p[l2["b"]:l2["b"] + 32] = 0.0
    p[l2["b"] + 32:l2["b"] + 64] = -20.0


def test_act_grad_image_on_both_branches_and_the_boundary(dev):
    T, N, E, MB = 2, 4096, 2, 4096
    a, rows, (P0, C0) = _update(dev, 0, T, N, E, MB, prof=True, edit=_act_edge)
    b, _, _ = _update(dev, 1, T, N, E, MB, edit=_act_edge)
    assert _tail_launches(rows, MB) == 2 * E * (T * N // MB)
    _assert_identical(a, b)
    ps = nets.make_spec("B", O, 6, True)
    l2 = ps.layers[1]
    # the columns at h2 = 0 took the gradient of act' = 1 (the h2 + 1 side of the select at its boundary) and trained
    assert (a[0][l2["b"]:l2["b"] + 32] - P0[l2["b"]:l2["b"] + 32]).abs().max().item() > 1e-5


def test_no_effect_on_four_waves(dev):
    T, N, E, MB = 2, 4096, 2, 4096
    a, rows_a, _ = _update(dev, 0, T, N, E, MB, waves=4, prof=True)
    b, rows_b, _ = _update(dev, 1, T, N, E, MB, waves=4, prof=True)
    assert _tail_launches(rows_a, MB) == 2 * E * (T * N // MB) and _tail_launches(rows_b, MB) == 2 * E * (T * N // MB)
    _assert_identical(a, b)


def test_option_takes_zero_or_one_only(dev):
    c = Ctx(0)
    try:
        for bad in (2, -1, 4, 8):
            with pytest.raises(Exception):
                c.set_option("tail32_lean", bad)
        c.set_option("tail32_lean", 0)
        c.set_option("tail32_lean", 1)
    finally:
        c.close()
