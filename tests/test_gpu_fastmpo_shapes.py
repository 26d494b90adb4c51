"""GPU: fastmpo.hip across the slots of its hand-indexed kernels, each case one rlx_fastmpo_update_f32 call against the float64 twin
(tests/fastmpo_twin.py) at the bars of tests/fastmpo_cases.py.

| case      | kinds (policy / critic) | widths (critic)   | E | NA  | A  | K  | B            | what it is there for                                        |
|-----------|-------------------------|-------------------|---|-----|----|----|--------------|-------------------------------------------------------------|
| two_atoms | mpo / mpo               | 64                | 1 | 2   | 1  | 1  | 5            | the smallest support, one lane of action, one sample (both  |
|           |                         |                   |   |     |    |    |              | weight softmaxes 1), sample_l1<4, LayerNorm, tanh> NJ 1     |
| act64     | fastsac / fastsac       | 64                | 2 | 65  | 64 | 7  | 6            | every action lane, the second atom slot by one atom, an odd |
|           |                         |                   |   |     |    |    |              | K, the clipped choice, k_mpo_dual at A 64                   |
| defaults  | fastsac / fastsac       | 768, 384, 192     | 2 | 101 | 3  | 64 | 8            | the reference's networks (mixed widths, NJ 12 in the norm   |
|           |                         | policy 512,256,128|   |     |    |    |              | kernels, sample_l1<12> NJ 12), every sample lane            |
| wide      | fasttd3 / fasttd3       | 1024, 64, 64      | 2 | 128 | 5  | 7  | 8            | sample_l1<16> NJ 16, every atom slot, (none, ReLU)          |
| tanh512   | mpo / mpo               | 512, 256, 128     | 1 | 51  | 5  | 4  | 8            | sample_l1<8, LayerNorm, tanh> NJ 8, the mean over critics   |
|           |                         |                   |   |     |    |    |              | path with one critic                                        |
| edges     | fastsac / fasttd3       | 128, 64, 64       | 2 | 51  | 5  | 4  | 13           | targets past both support edges: v +-100, rewards +-500     |
|           |                         |                   |   |     |    |    |              | (a support away from the default: the expected-q floor 10)  |
| many_rows | fastsac / fastsac       | 64 (policy 128)   | 1 | 11  | 2  | 2  | 64 CUs + 37  | past the row-grid caps (rows_grid 8 x CUs workgroups of 4   |
|           |                         |                   |   |     |    |    |              | rows, bwd_rows_grid 4 x CUs of 16); B >= 4096: the critics' |
|           |                         |                   |   |     |    |    |              | weight gradients on the split-operand engine                |
| split     | fastsac / fastsac       | 128               | 2 | 51  | 5  | 4  | 1024         | K B = 4096 target rows: hidden layers 2 and 3 of the target |
|           |                         |                   |   |     |    |    |              | critics on the split-operand images                         |

The profiler confirms the engine choices (k_gemm_fwd / k_gemm_dw rows, `engine` 1 = split-operand), the way test_gpu_mpo_shapes.py
does: the target critics' hidden layers on engine 1 exactly when their row count is >= 4096; the policy's weight gradients on
engine 0 whatever their row count."""
import numpy as np
import pytest
import torch

import fastmpo_cases as fc
from fastmpo_cases import Case, Run

pytestmark = pytest.mark.gpu


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(name):
    if name == "two_atoms":
        return Case(201, "mpo", E=1, NA=2, A=1, K=1, B=5, P=1, G=2, policy_hidden=(64, 64, 64), critic_hidden=(64, 64, 64), action_clipping=True)
    if name == "act64":
        return Case(202, "fastsac", E=2, NA=65, A=64, K=7, B=6, P=1, G=2, policy_hidden=(64, 64, 64), critic_hidden=(64, 64, 64),
                    clipped_double_q_learning=True, action_clipping=True)
    if name == "defaults":
        return Case(203, "fastsac", E=2, NA=101, A=3, K=64, B=8, P=1, G=2, policy_hidden=(512, 256, 128), critic_hidden=(768, 384, 192))
    if name == "wide":
        return Case(204, "fasttd3", E=2, NA=128, A=5, K=7, B=8, P=1, G=2, policy_hidden=(1024, 64, 64), critic_hidden=(1024, 64, 64),
                    clipped_double_q_learning=True)
    if name == "tanh512":
        return Case(205, "mpo", E=1, NA=51, A=5, K=4, B=8, P=1, G=2, policy_hidden=(512, 256, 128), critic_hidden=(512, 256, 128))
    if name == "edges":
        c = Case(206, "fasttd3", policy_kind="fastsac", E=2, B=13, P=1, G=2, clipped_double_q_learning=True, v_min=-100.0, v_max=100.0)
        r = c.batches[3]
        r[:] = np.where(np.arange(r.size).reshape(r.shape) % 2 == 0, 500.0, -500.0)      # past both edges of v +-100
        return c
    if name == "many_rows":
        # (K 2 and policy widths apart from the critic's: no other GEMM of the call has a target pass's (M, N, K))
        return Case(207, "fastsac", E=1, NA=11, A=2, K=2, B=64 * _num_cus() + 37, P=1, G=1, policy_hidden=(128, 128, 128),
                    critic_hidden=(64, 64, 64))
    if name == "split":
        return Case(208, "fastsac", E=2, NA=51, A=5, K=4, B=1024, P=1, G=1, policy_hidden=(128, 128, 128), critic_hidden=(128, 128, 128))
    raise KeyError(name)


# The critics' parameter step of `defaults` (768-384-192 LayerNorm critics on 8 rows, the SECOND Adam step, where the moments no
# longer cancel rounding) measures 2.6e-4 against the twin on an MI355X; the bar is 1.5 x that measurement.  That the figure is
# the number format's and not the library's: the twin's own arithmetic run in float32 by torch on the CPU is 3.3e-4 from the float64
# twin (tests/test_fastmpo_twin.py::test_float32_step_gap_of_the_widest_case).  Every other figure of the case keeps the project's bar.
STEP_TOL = {"defaults": 4e-4}
NAMES = ["two_atoms", "act64", "defaults", "wide", "tanh512", "edges", "many_rows", "split"]


def _gemm_rows(ctx, fn):
    ctx.prof_begin()
    try:
        r = fn()
    finally:
        ctx.prof_end()
    return r, [q for q in ctx.prof_rows() if q["kernel"] in ("k_gemm_fwd", "k_gemm_dw")]


def _check_engines(ctx, c, rows):
    """the engine of the target critics' hidden layers 2 and 3 (critic step: K B rows; policy step: K 2B rows) and of the weight
    gradients, as the selection code decides it"""
    bx = ctx.get_counter("gemm_bx") == 1
    B, R, K = c.B, 2 * c.B, c.K
    h = c.LQ["hidden"]
    if not bx:
        assert all(q["engine"] == 0 for q in rows), rows
    for T in (K * B, K * R):
        for l in (1, 2):
            got = {q["engine"] for q in rows if q["kernel"] == "k_gemm_fwd" and (q["M"], q["N"], q["K"]) == (T, h[l], h[l - 1])}
            assert got == {1 if bx and T >= 4096 else 0}, (got, T, l)
    ph = c.LP["hidden"]
    pol = {q["engine"] for q in rows if q["kernel"] == "k_gemm_dw" and q["K"] == R and q["N"] in ph}
    assert pol == {0}, (pol, R)                                  # the actor's weight gradients: always the exact engine
    cri = {q["engine"] for q in rows if q["kernel"] == "k_gemm_dw" and q["K"] == B and q["N"] in h}
    assert cri == {1 if bx and B >= 4096 else 0}, (cri, B)


@pytest.mark.parametrize("name", NAMES)
def test_one_update_matches_the_twin(ctx, dev, name):
    c = _case(name)
    nc = _num_cus()
    claims = {"two_atoms": lambda: c.NA == 2 and c.A == 1 and c.K == 1,
              "act64": lambda: c.NA == 65 and c.A == 64 and c.K == 7,
              "defaults": lambda: c.LQ["hidden"] == (768, 384, 192) and c.K == 64 and c.NA == 101 and c.B == 8,
              "wide": lambda: c.LQ["hidden"][0] == 1024 and c.LP["hidden"][0] == 1024 and c.NA == 128,
              "tanh512": lambda: c.LQ["hidden"][0] == 512 and c.E == 1,
              "edges": lambda: c.h["v_max"] == 100.0 and c.h["v_min"] == -100.0 and c.batches[3].max() > c.h["v_max"] * (1 + c.h["gamma"]) and
              c.batches[3].min() < c.h["v_min"] * (1 + c.h["gamma"]),
              "many_rows": lambda: -(-c.B // 4) > 8 * nc and -(-2 * c.B // 16) > 4 * nc and c.B >= 4096 and c.B % 4 != 0,
              "split": lambda: c.K * c.B == 4096 and 2 * c.B < 4096}[name]
    assert claims(), name
    new, met, counts, ex = c.twin()
    if name == "edges":                                        # every projected target sits on an edge atom
        t = ex["critic"]["target"]
        assert float((t[..., 0] + t[..., -1]).min()) > 1.0 - 1e-12
    r, rows = _gemm_rows(ctx, lambda: Run(ctx, dev, c))
    fc.check_against_twin(r, new, met, counts, c.h, c.st, STEP_TOL.get(name, 2e-4), fc.min_selected(c))
    _check_engines(ctx, c, rows)
