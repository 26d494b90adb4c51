#!/usr/bin/env python
"""Tuning aid: phase stamps (clock64 of thread 0, workgroup 0) of k_tail32_bx at the bench minibatch, for four and eight waves
per tile (option tail32_waves) and, on eight waves, the earlier and the lean form (option tail32_lean = 0 / 1) alternated twice in
one process -- the stamps sit at the same source positions in both ("metric sums" is one barrier in the lean form; its serial
sections and its act'(H2) image run on waves 4-7, which thread 0 does not stamp: read the whole tile).
Needs a library built with the stamps compiled in:
    RLX_BUILD_TAG=t32s RLX_EXTRA_DEFINES=-DRLX_T32_STAMPS=1 python rl-x_amd/build.py
    RLX_HIP_LIBRARY=rl-x_amd/lib/librlxhip_t32s.so python tools/tail32_phases.py [minibatch rows]
The per-phase entry runs the two networks' chains on two streams, as the update does; the stamps are those of the launch that
wrote last (workgroup 0 is among the first on the chip, so its neighbours are its own launch's workgroups and the other chain's)."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd")); sys.path.insert(0, ROOT)
import torch
from rlx_amd.hip import Ctx, PpoHparams, mlp_desc
dev = torch.device("cuda:0")
ctx = Ctx(0)
O, A, B, mb = 17, 6, 524288, int(sys.argv[1]) if len(sys.argv) > 1 else 32768
pd = mlp_desc(O, [512, 256, 128], A, 1, True, True)
cd = mlp_desc(O, [512, 256, 128], 1, 1, True, False)
npar, ncar = ctx.lib.rlx_mlp_param_count(ctypes.byref(pd)), ctx.lib.rlx_mlp_param_count(ctypes.byref(cd))
P, C = torch.randn(npar, device=dev) * 0.05, torch.randn(ncar, device=dev) * 0.05
P[-A:] = 0
states, actions = torch.randn(B, O, device=dev), torch.randn(B, A, device=dev)
logp, ret, adv = torch.randn(B, device=dev) * 0.1 - 8, torch.randn(B, device=dev), torch.randn(B, device=dev)
idx = torch.randperm(B, device=dev)[:mb].to(torch.int32)
pg, cg, met = torch.zeros(npar, device=dev), torch.zeros(ncar, device=dev), torch.zeros(8, device=dev)
hp = PpoHparams(0.1, 0.0, 1.0, 5.0, 0.9, 0.999, 1e-8)
ctx.set_option("ppo_tail", 2)
names = ["H2 request + split + plane stores", "barrier", "phase A K loop", "act + H3 tile stores", "barrier",
         "head + loss + seeds", "metric sums (two barriers)", "head dW partials + barrier + sums", "barrier", "dZ3",
         "barrier", "phase C K loop", "dZ2 epilogue"]
for waves, lean in ((4, 0), (8, 0), (8, 1), (8, 0), (8, 1)):
    ctx.set_option("tail32_waves", waves)
    ctx.set_option("tail32_lean", lean)
    for _ in range(3):
        ctx.ppo_minibatch_fwd_bwd(pd, P, pg, cd, C, cg, met, states, actions, logp, ret, adv, idx, hp)
    runs = []
    for _ in range(5):
        st = torch.zeros(16, dtype=torch.int64, device=dev)
        ctx.dbg_set_stamps(st)
        ctx.ppo_minibatch_fwd_bwd(pd, P, pg, cd, C, cg, met, states, actions, logp, ret, adv, idx, hp)
        torch.cuda.synchronize()
        ctx.dbg_set_stamps(None)
        runs.append(st.cpu().numpy().astype("int64"))
    s = sorted(runs, key=lambda r: int(r[13] - r[0]))[len(runs) // 2]          # the median run by total ticks
    if int(s[13]) == 0:
        raise SystemExit("no stamps: build with -DRLX_T32_STAMPS=1 and select the library with RLX_HIP_LIBRARY")
    d = [int(s[i + 1] - s[i]) for i in range(13)]
    ticks, wall_us = int(s[13] - s[0]), (int(s[15]) - int(s[14])) / 100.0
    print(f"k_tail32_bx, {waves} waves per tile, tail32_lean = {lean}, mb {mb}: workgroup 0's tile = {ticks} clock64 ticks in {wall_us:.2f} us of wall_clock64"
          f" -> {ticks / max(wall_us, 1e-9) / 1e3:.2f} GHz   (totals of 5 runs: {' '.join(str(int(r[13] - r[0])) for r in runs)})")
    for n, v in zip(names, d):
        print(f"    {n:40s} {v:7d}  {100.0 * v / ticks:5.1f} %")
