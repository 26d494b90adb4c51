"""k_gemm_fwd (rlx_dbg_gemm_f32 mode 0) against the split-K kernel for few rows (mode 6, gemm_sk.hip) and torch.mm + bias + relu on the
same tensors: N = 512, M in {8, 32, 128, 256, 512, 1024}, K in {512, 2048, 3136} -- among them the reference's three shapes, dqn's
and pqn's hidden Dense [32 | 8, 3136] and the SimbaV2 block's second product [256, 2048].  tools/ens_bench.py's event timer after a
warm-up; the three routes alternate, twice in every run (the second figure is kept), and a timed window is --iters calls.  The rule
of gemm_fwd_auto (M*, K*: DESIGN.md section 4.5r) is read off this table: a shape is in it where mode 6 beats mode 0 by more than
the spread between the runs.  Measurement only: one JSON line per run, no pass / fail; the largest difference between the two
kernels' outputs is printed so that a wrong result cannot post a time.

    python tools/gemm_small_m_bench.py [--warmup 20] [--iters 2000] [--runs 2] [--slices 0]
"""
import argparse
import json

import torch

from ens_bench import timed
from rlx_amd.hip import ACT_RELU, Ctx

N, ROWS, KS = 512, (8, 32, 128, 256, 512, 1024), (512, 2048, 3136)


def one_run(a, ctx, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {}
    for K in KS:
        W, b = (torch.randn(K, N, generator=g) * 0.05).to(dev), torch.randn(N, generator=g).to(dev)
        for M in ROWS:
            A, C0, C6 = torch.randn(M, K, generator=g).to(dev), torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
            t = lambda f: round(1e3 * timed(f, a.warmup, a.iters), 2)
            k = f"m{M}_k{K}"
            for _ in range(2):      # the routes alternate
                res[f"fwd_us_{k}"] = t(lambda: ctx.dbg_gemm(0, A, W, C0, b, M, N, K, ACT_RELU))
                res[f"sk_us_{k}"] = t(lambda: ctx.dbg_gemm(6, A, W, C6, b, M, N, K, ACT_RELU))
                res[f"torch_us_{k}"] = t(lambda: torch.relu(torch.addmm(b, A, W)))
            res[f"max_abs_diff_{k}"] = float((C0 - C6).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("warmup", 20), ("iters", 2000), ("runs", 2), ("slices", 0)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev, ctx = torch.device("cuda:0"), Ctx(0)
    ctx.set_option("gemm_sk_slices", a.slices)
    for _ in range(a.runs):
        print(json.dumps(one_run(a, ctx, dev)), flush=True)


if __name__ == "__main__":
    main()
