"""GPU: the projection of weight matrices to unit column norm (hyper.hip) -- rlx_colnorm_f32 over the strip shapes (N below one strip,
several strips, tall matrices, N no multiple of 4: the one-column-per-lane path, E > 1) and rlx_hyper_project_f32 on a network's flat
parameter vector -- against W[:, n] / max(|W[:, n]|, 1e-8) in float64; bars by tests/test_gpu_hyper_net.py's formula."""
import pytest
import torch

from test_gpu_hyper_net import CASES, EPS, case, check, layout, split

#        K, N, E
SHAPES = [(12, 64, 1), (512, 2048, 2), (2048, 512, 2), (128, 101, 1), (65, 6, 2)]


def ref_colnorm(W, dt):
    W = W.to(dt)
    return W / W.norm(dim=-2, keepdim=True).clamp_min(EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_colnorm_matches_float64_and_keeps_a_zero_column(ctx, dev, shape):
    K, N, E = shape
    W = torch.randn(E, K, N, generator=torch.Generator().manual_seed(K + N)) * 3
    W[E - 1, :, N // 2] = 0
    got = W.to(dev)
    ctx.colnorm(got)
    check(shape, "W", got.cpu(), ref_colnorm(W, torch.float64), ref_colnorm(W, torch.float32))
    assert not got[E - 1, :, N // 2].any()


@pytest.mark.gpu
def test_project_normalises_the_matrices_and_leaves_scalers_bit_identical(ctx, dev):
    c = CASES[1]
    _, in_dim, H, blocks = c
    (desc, params, _, _), _, _ = case(c)
    params = params * 1.7      # (the case's matrices are projected already)
    got = params.to(dev)
    ctx.hyper_project(desc, got)
    g, p = split(got.cpu(), in_dim, H, blocks), split(params, in_dim, H, blocks)
    for name, shp in layout(in_dim, H, blocks):
        if len(shp) == 2:
            check(c, name, g[name], ref_colnorm(p[name], torch.float64), ref_colnorm(p[name], torch.float32))
        else:
            assert torch.equal(g[name], p[name]), name
