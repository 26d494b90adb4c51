#!/usr/bin/env python
"""Tuning aid: phase stamps (clock64 of thread 0, workgroup 0) of k_dx_l1bwd<2, 8, ELU, LN, BX> at the bench minibatch, every kernel
alone on the chip, in the two forms of a library option alternated twice in one process: by default l1_stats_handover = 0 (the
LayerNorm row statistics rebuilt from the recomputed z1) and = 1 (loaded from the array k_l12fwd left: k_dx_l1bwd_stats); with
l1_wrap_refill the handover form's K loop with the conditional refill (0: k_dx_l1bwd_stats) and with unconditional refills that wrap
into the first-layer image (1: k_dx_l1bwd_stats_wrap) -- the stamps sit at the same source positions in both.  A stamp does not wait
for what was issued before it, so a boundary moves with the loads: read the whole tile and the sum of the first three phases.
Needs a library built with the stamps compiled in: RLX_EXTRA_DEFINES=-DRLX_LF_STAMPS=1 python rl-x_amd/build.py --force
    python tools/dx_phases.py [minibatch rows, default 32768] [option, default l1_stats_handover; e.g. ln_row_once, l1_wrap_refill]"""
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
OPTION = sys.argv[2] if len(sys.argv) > 2 else "l1_stats_handover"
RED1 = "reduction 1 (partials, barrier, fold, row statistics)"
HAND1 = "statistics loaded (first tile: dW1 scale)"      # the handover form has no first reduction: the stamp follows the z1 recompute's
REPS = 5
for form in (0, 1, 0, 1):
    ctx.set_option(OPTION, form)
    names = ["tile start (top barrier, next tile's loads issued)", "K loop + rescale + next tile's stage store", "z1 recompute",
             HAND1 if ((OPTION == "l1_stats_handover" and form == 1) or OPTION == "l1_wrap_refill") else RED1, "element-wise loop 1", "reduction 2 (barrier, fold)",
             "element-wise loop 2", "dW1 product (issue)"]
    for _ in range(3):
        ctx.ppo_minibatch_fwd_bwd(pd, P, pg, cd, C, cg, met, states, actions, logp, ret, adv, idx, hp)
    acc, ghz = [0] * 16, 0.0
    for _ in range(REPS):
        st = torch.zeros(20, dtype=torch.int64, device=dev)
        ctx.dbg_set_stamps(st)
        ctx.ppo_minibatch_fwd_bwd(pd, P, pg, cd, C, cg, met, states, actions, logp, ret, adv, idx, hp)
        torch.cuda.synchronize()
        ctx.dbg_set_stamps(None)
        s = st.cpu().numpy()
        if int(s[16]) == 0:
            sys.exit("no stamps: build the library with RLX_EXTRA_DEFINES=-DRLX_LF_STAMPS=1")
        for i in range(16):
            acc[i] += int(s[i + 1] - s[i])
        ghz += int(s[16] - s[0]) / ((int(s[19]) - int(s[18])) / 100.0) / 1e3
    d = [v / REPS for v in acc]
    print(f"{OPTION} = {form}: k_dx_l1bwd workgroup 0 (the critic's launch), mb {mb}, mean of {REPS} launches: two tiles = {sum(d):.0f} clock64 ticks at {ghz / REPS:.2f} GHz")
    for t in range(2):
        print(f"  tile {t}: " + ", ".join(f"{n} {v:.0f}" for n, v in zip(names, d[8 * t:8 * t + 8])))
    print(f"  tile 1, tile start + K loop + z1 recompute: {sum(d[8:11]):.0f} ticks; element-wise phases (reduction 1 .. loop 2): {sum(d[11:15]):.0f} ticks; whole tile {sum(d[8:16]):.0f}")
