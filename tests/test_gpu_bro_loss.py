"""GPU: rlx_bro_quantile_loss_f32 (bro.hip) -- loss, dq1, dq2 and y_out -- against include/rlx_hip.h's formulas (bro.py:29-32,
:179-189) as a plain torch function on the CPU in float64 with autograd; bars as tests/test_gpu_hyper_net.py's `check`.

(1, 1): one lane, one term.  (5, 25): a ragged workgroup (four rows per workgroup), N below a wave.  (128, 100): the reference's
batch and quantiles, lanes that own two quantiles.  (3, 128): the widest row.  Row 0 of every case has term = 1 (y = r).

The function has kinks at td = 0 and |td| = kappa.  Inputs are continuous draws from fixed seeds; for these seeds the float32
function has every td on float64's side of every kink (`same_side`, verified on the CPU; the test asserts it again before it
compares, and no element is excluded)."""
import functools

import pytest
import torch

from test_gpu_hyper_net import check

CASES = [(B, N, pess) for B, N in ((1, 1), (5, 25), (128, 100), (3, 128)) for pess in (0.0, 0.5)]
GAMMA, KAPPA = 0.99, 1.0


def ref_loss(dt, q1, q2, n1, n2, rew, term, nlogp, log_alpha, pess):
    q1, q2 = (q.to(dt).clone().requires_grad_() for q in (q1, q2))
    n1, n2, rew, term, nlogp, log_alpha = (t.to(dt) for t in (n1, n2, rew, term, nlogp, log_alpha))
    B, N = q1.shape
    nq = (n1 + n2) / 2 - pess * (n1 - n2).abs() / 2
    y = rew[:, None] + (GAMMA * (1 - term))[:, None] * (nq - (log_alpha.exp() * nlogp)[:, None])
    tau = (torch.arange(N, dtype=dt) + 0.5) / N
    loss, tds = 0, []
    for q in (q1, q2):
        td = y[:, None, :] - q[:, :, None]      # [B, i, j]
        huber = torch.where(td.abs() <= KAPPA, 0.5 * td ** 2, KAPPA * (td.abs() - 0.5 * KAPPA))
        loss = loss + ((tau[None, :, None] - (td < 0).to(dt)).abs() * huber / KAPPA).sum() / (B * N)
        tds.append(td.detach())
    loss.backward()
    return dict(loss=loss.detach().reshape(1), dq1=q1.grad, dq2=q2.grad, y=y, td=torch.stack(tds))


@functools.lru_cache(maxsize=None)
def case(c):
    B, N, pess = c
    g = torch.Generator().manual_seed(100 * B + N)
    r = lambda *s: torch.randn(*s, generator=g)
    term = (torch.rand(B, generator=g) < 0.2).float()
    term[0] = 1.0
    inp = (r(B, N), r(B, N), r(B, N), r(B, N), r(B), term, r(B) - 1.0, torch.tensor([-0.7]), pess)
    return inp, ref_loss(torch.float64, *inp), ref_loss(torch.float32, *inp)


def same_side(r64, r32):
    sides = lambda td: torch.stack([td < 0, td.abs() <= KAPPA])
    return bool((sides(r64["td"]) == sides(r32["td"])).all())


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=str)
def test_loss_gradients_and_targets_match_float64(ctx, dev, c):
    B, N, pess = c
    inp, r64, r32 = case(c)
    assert same_side(r64, r32), "the float32 reference crosses a kink: change the seed"
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    dq1, dq2, loss, y = nan(B, N), nan(B, N), nan(1), nan(B, N)
    ctx.bro_quantile_loss(*(t.to(dev) for t in inp[:8]), GAMMA, pess, KAPPA, dq1, dq2, loss, y)
    got = dict(loss=loss, dq1=dq1, dq2=dq2, y=y)
    worst = max(check(c, k, got[k].cpu(), r64[k], r32[k]) for k in got)
    print(f"{c}: worst fraction of a bar {worst:.3f}")
