#!/usr/bin/env python
"""Tuning aid: phase stamps (clock64 of thread 0, workgroup 0) of k_l12fwd at the bench minibatch, every kernel alone on the chip, in
the two forms of a library option alternated twice in one process: by default l12_prefetch = 0 (k_l12fwd: first-layer fragments and
the next tile's observations loaded at the tile top) and = 1 (k_l12fwd_pf: the fragments in registers when the tile starts, the
observations requested behind them and staged behind the K loop) -- the stamps sit at the same source positions in both.  A stamp
does not wait for what was issued before it, so a boundary moves with the loads: read the whole tile next to the single phases.
Needs a library built with the stamps compiled in: RLX_EXTRA_DEFINES=-DRLX_L12_STAMPS=1 python rl-x_amd/build.py --force
    python tools/l12_phases.py [minibatch rows, default 32768] [option, default l12_prefetch; e.g. ln_row_once, l1_stats_handover]
(Until round 10 the second and third argument were VALUES of ln_row_once and l1_stats_handover, set together for one run.  That
setup is no longer reachable from the command line: one option alternates, every other option keeps the library's default.)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd")); sys.path.insert(0, ROOT)
import torch
from rlx_amd.hip import Ctx, PpoHparams, mlp_desc
dev = torch.device("cuda:0")
ctx = Ctx(0)
O, A, B, mb = 17, 6, 524288, int(sys.argv[1]) if len(sys.argv) > 1 else 32768
OPTION = sys.argv[2] if len(sys.argv) > 2 else "l12_prefetch"
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
names = ["prologue", "z1 MFMA + next x stage", "LN sums + barrier", "normalise + ELU + h1 store + image + barrier", "layer-2 K loop",
         "h2 epilogue + store", "loop-top barrier"]
if OPTION == "l12_prefetch":      # with 1 the next tile's observations are staged behind the K loop: that stage store moves between two phases
    names[1], names[4] = "z1 MFMA (+ next x stage with 0)", "layer-2 K loop (+ next x stage with 1)"
REPS = 5
for form in (0, 1, 0, 1):
    ctx.set_option(OPTION, form)
    for _ in range(3):
        ctx.ppo_minibatch_fwd_bwd(pd, P, pg, cd, C, cg, met, states, actions, logp, ret, adv, idx, hp)
    acc, ghz, wall = [0] * 12, 0.0, 0.0
    for _ in range(REPS):
        st = torch.zeros(16, dtype=torch.int64, device=dev)
        ctx.dbg_set_stamps(st)
        ctx.ppo_minibatch_fwd_bwd(pd, P, pg, cd, C, cg, met, states, actions, logp, ret, adv, idx, hp)
        torch.cuda.synchronize()
        ctx.dbg_set_stamps(None)
        s = st.cpu().numpy()
        if int(s[12]) == 0:
            sys.exit("no stamps: build the library with RLX_EXTRA_DEFINES=-DRLX_L12_STAMPS=1 (and at least two tiles per workgroup)")
        for i in range(12):
            acc[i] += int(s[i + 1] - s[i])
        w = (int(s[15]) - int(s[14])) / 100.0
        wall += w
        ghz += int(s[12] - s[0]) / w / 1e3
    d = [v / REPS for v in acc]
    print(f"{OPTION} = {form}: k_l12fwd workgroup 0 (the critic's launch), mb {mb}, mean of {REPS} launches: two tiles = {sum(d):.0f} clock64 ticks "
          f"in {wall / REPS:.2f} us of wall_clock64 -> {ghz / REPS:.2f} GHz")
    print("  tile 0: " + ", ".join(f"{n} {v:.0f}" for n, v in zip(names, d[:7])))
    print("  tile 1: " + ", ".join(f"{n} {v:.0f}" for n, v in zip(names[1:6], d[7:12])))
    print(f"  tile 0 without its prologue (z1 .. h2 store): {sum(d[1:6]):.0f} ticks; tile 1 with the barrier in front of it: {sum(d[6:12]):.0f} ticks")
