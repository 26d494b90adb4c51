"""GPU: the schedules of the PPO whole-update calls (rlx_ppo_update_f32 / rlx_ppo_update_dist_f32, rl-x_amd/csrc/ppo.hip) agree bit
for bit.  Twin launches on one stream, two free-running chains with grouped gathers, with the parity double buffer or with a
gather per chain (own_rows), and the sequential per-update path all issue the same kernels per network, on the same rows, in the
same order, and a gather is a pure copy: whichever way the options route a call, both parameter vectors, all four moment vectors
and the metric rows must come out identical.  The cases are the smallest that reach every branch of the schedules: three gather
groups with a short last one (the third group waits for the critic's last read of the first), four updates through the two
parity buffers, one rank that holds every row against the local call, and a ragged shard whose grouped gathers carry per-update
valid-row counts."""
import numpy as np
import pytest
import torch

from rlx_amd.hip import Ctx, PpoHparams
from rlx_amd.hip import lib as L
from test_gpu_dist import _nets, _rollout

pytestmark = pytest.mark.gpu

DEFAULTS = {"ppo_twin": -1, "gather_group_rows": 524288, "gather_records": 1, "two_streams": 1}
HP = PpoHparams(0.1, 0.0, 1.0, 5.0, 0.9, 0.999, 1e-8)
NAMES = ("policy", "policy m", "policy v", "critic", "critic m", "critic v", "metrics")


def _update(c, dev, nets, roll, E, mb, opts, dist=None):
    """one whole update from fresh moments under the options `opts`; dist = (n_global, env offset) takes the data-parallel entry.
    Returns (policy, m, v, critic, m, v, metrics)."""
    _, _, pd, cd, P0, C0 = nets
    T, n_local = roll[2].shape
    n_upd = E * (T * (dist[0] if dist else n_local) // mb)
    lr = np.linspace(4e-4, 1e-4, n_upd).astype(np.float32)
    P, C, met = P0.clone(), C0.clone(), torch.empty(n_upd, 10, device=dev)
    pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, P, C, C))
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        if dist:
            _, cnt = c.ppo_update_dist(pd, P, pm, pv, cd, C, cm, cv, *roll, dist[0], dist[1], E, mb, L.prng_key(5), 0, lr, HP, met)
        else:
            _, cnt = c.ppo_update(pd, P, pm, pv, cd, C, cm, cv, *roll, E, mb, L.prng_key(5), 0, lr, HP, met)
        torch.cuda.synchronize()
    finally:
        for k in opts:
            c.set_option(k, DEFAULTS[k])
    assert cnt == n_upd and bool(torch.isfinite(met).all())
    return P, pm, pv, C, cm, cv, met


def _same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), (what, name, (x - y).abs().max().item())


def test_local_two_chains_groups_of_three(ctx, dev):
    """8 updates of 1024 rows; gather_group_rows = 3072: groups of 3, 3 and 2 updates.  Against one gather per chain and update
    (own_rows), the five-array gather, and the sequential path."""
    T, N, mb, E = 16, 256, 1024, 2
    nets, roll = _nets(dev), _rollout(dev, T, N)
    run = lambda **o: _update(ctx, dev, nets, roll, E, mb, dict(ppo_twin=0, **o))
    grouped = run(gather_group_rows=3072)
    _same(grouped, run(gather_group_rows=0), "own_rows")
    _same(grouped, run(gather_group_rows=3072, gather_records=0), "no records")
    _same(grouped, run(gather_group_rows=3072, two_streams=0), "sequential")


def test_local_two_chains_parity_double_buffer(ctx, dev):
    """4 updates of 16384 rows with one gather per update (too large for own_rows): the row buffers alternate by update parity and
    the gather of update 2 waits for the critic's read of update 0.  Against the grouped default."""
    T, N, mb, E = 16, 2048, 16384, 2
    nets, roll = _nets(dev), _rollout(dev, T, N)
    run = lambda **o: _update(ctx, dev, nets, roll, E, mb, dict(ppo_twin=0, **o))
    _same(run(gather_group_rows=0), run(), "parity buffers against groups")


@pytest.fixture(scope="module")
def shape20(dev):
    """20 updates of 4096 rows: with groups of 32768 rows, gathers of 8, 8 and 4 updates"""
    T, N = 16, 1024
    return _nets(dev), _rollout(dev, T, N), 5, 4096, N


def test_local_twin_three_groups(ctx, dev, shape20):
    """twin launches with the rows of 8 updates per gather launch, from the row records and from the five arrays"""
    nets, roll, E, mb, _ = shape20
    run = lambda **o: _update(ctx, dev, nets, roll, E, mb, dict(ppo_twin=1, **o))
    _same(run(), run(gather_records=0), "twin: records against the five arrays")


@pytest.mark.parametrize("twin", [1, 0])
def test_dist_one_rank_equals_local(ctx, dev, shape20, twin):
    """a rank that holds every row: the data-parallel entry is the local one (for the two chains with the same 8 updates per
    gather group on both sides), with and without the row records"""
    nets, roll, E, mb, N = shape20
    local = _update(ctx, dev, nets, roll, E, mb, dict(ppo_twin=twin, gather_group_rows=524288 if twin else 32768))
    dist = _update(ctx, dev, nets, roll, E, mb, dict(ppo_twin=twin), dist=(N, 0))
    _same(dist, local, "dist against local")
    _same(dist, _update(ctx, dev, nets, roll, E, mb, dict(ppo_twin=twin, gather_records=0), dist=(N, 0)), "dist: no records")


@pytest.mark.parametrize("twin,T,NG,mb,E", [(0, 16, 512, 2048, 24), (1, 16, 2048, 8192, 6)])
def test_dist_ragged_shard_grouped_gathers(dev, twin, T, NG, mb, E):
    """rank 1 of 2: ragged local minibatches padded to the capacity, more than three gather groups of per-update valid-row counts.
    A context of world 2 refuses to run without a communicator, so a hook that leaves the buffers alone stands in for the
    collectives (they are issued, with the all-reduce in front of clip + Adam; nothing is added): both sides see this rank's
    partial statistics and gradients only, and must agree with each other."""
    me = Ctx(0)
    try:
        me.set_rank(1, 2)
        me.set_allreduce_hook(lambda ptr, n, dtype, on_side: None)
        NL = NG // 2
        cap = me.dist_row_capacity(mb, NL, NG)
        n_upd = E * (T * NG // mb)
        assert n_upd * cap > 3 * 32768 and cap < mb and (not twin or cap >= 4096)
        nets = _nets(dev, seed=2)
        mine = tuple(x[:, NL:].contiguous() for x in _rollout(dev, T, NG, seed=2))
        rec = _update(me, dev, nets, mine, E, mb, dict(ppo_twin=twin), dist=(NG, NL))
        _same(rec, _update(me, dev, nets, mine, E, mb, dict(ppo_twin=twin, gather_records=0), dist=(NG, NL)), "ragged: no records")
        assert me.dist_overflow_counts() == (0, 0)
    finally:
        me.set_allreduce_hook(None)
        me.close()
