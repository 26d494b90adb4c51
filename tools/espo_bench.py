"""Time ESPO's epoch loop (rlx_espo_update_f32) at the reference's default shape (obs 48, act 12, hidden 256, minibatches of 64 rows
out of 8192) on one MI355X: the time per executed epoch at chunk lengths 1, 2, 4 and 16 with one and with two streams, the cost of an
early stop (epoch 10 of 300), and, for context, one 64-row rlx_ppo_minibatch_fwd_bwd_f32 with its two clip + Adam calls.

    python tools/espo_bench.py [--epochs 64] [--plan PLAN]          # event / wall-clock timings, one JSON line each
    rocprofv3 --kernel-trace -d DIR -- python tools/espo_bench.py --plan PLAN           # the same run under the kernel trace
    python tools/espo_bench.py --db DIR/.../*_results.db --plan PLAN                     # per-call figures from that trace

Every rlx_espo_update_f32 call starts with exactly one k_espo_validate launch, and every epoch with one k_espo_gather: the trace is cut
into calls and epochs at those.  From the trace: launches per epoch, GPU span per executed epoch (first kernel start to last kernel
end of the call, over the epochs that were applied), and for the stopped call the span from the first kernel of the first wasted epoch
to the end of the call."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rl-x_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def analyse(db_path, plan):
    import sqlite3
    cur = sqlite3.connect(db_path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else "kernel_name"
    rows = cur.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    calls, cur_call = [], None
    for name, s, e in rows:
        if "k_espo_validate" in name:
            cur_call = []
            calls.append(cur_call)
        if cur_call is not None:
            cur_call.append((name, s, e))
    espo = [c for c in plan if c["what"] == "espo_update"]
    assert len(calls) == len(espo), (len(calls), len(espo))
    for c, ks in zip(espo, calls):
        # the call ends with its last ESPO-owned launch (the gated Adam of the last submitted epoch); what follows belongs to the tool
        last = max(i for i, k in enumerate(ks) if "k_espo_clip_adam" in k[0])
        ks = ks[:last + 1]
        gathers = [i for i, k in enumerate(ks) if "k_espo_gather" in k[0]]
        run, sub = c["epochs_run"], len(gathers)
        t0, t1 = ks[0][1], max(k[2] for k in ks)
        out = dict(c, epochs_submitted=sub, launches_per_epoch=round((len(ks) - 1) / sub, 2))
        if run < sub:
            w0 = ks[gathers[run]][1]
            out.update(gpu_us_per_executed_epoch=round((w0 - t0) / 1e3 / run, 2), gpu_us_after_stop=round((t1 - w0) / 1e3, 1),
                       wasted_epochs=sub - run)
        else:
            out["gpu_us_per_executed_epoch"] = round((t1 - t0) / 1e3 / run, 2)
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=64)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--db", default=None)
    args = ap.parse_args()
    if args.db:
        return analyse(args.db, json.load(open(args.plan)))
    import numpy as np
    import torch
    import espo_cases as ec
    from rlx_amd.hip import Ctx, PpoHparams
    dev = torch.device("cuda:0")
    ctx = Ctx(0)
    O, A, H, B, mb = 48, 12, 256, 8192, 64
    t = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt))).to(dev)
    plan = []

    def call(fc, label, E, thr, chunk, streams, timed=True):
        h = dict(fc.h, max_ratio_delta=thr)
        nets = [t(x) for x in (fc.p0, 0 * fc.p0, 0 * fc.p0, fc.c0, 0 * fc.c0, 0 * fc.c0)]
        pd, cd = ec.descs(fc)
        data = [t(x) for x in (fc.states, fc.actions, fc.log_probs, fc.returns, fc.advantages)]
        idx, met = t(fc.idx[:E], np.int32), torch.zeros(E, 8, device=dev)
        ctx.set_option("espo_chunk", chunk)
        ctx.set_option("two_streams", streams - 1)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        run, _ = ctx.espo_update(pd, nets[0], nets[1], nets[2], cd, nets[3], nets[4], nets[5], *data, idx, 0, h["learning_rate"], ec.espo_hp(h), met)
        ms = (time.perf_counter() - w0) * 1e3               # the call blocks at its end: wall clock == submission + GPU time
        rec = dict(what="espo_update", label=label, max_epochs=E, chunk=chunk, streams=streams, epochs_run=run, call_ms=round(ms, 3),
                   us_per_executed_epoch=round(ms * 1e3 / run, 2))
        plan.append(rec)
        if timed:
            print(json.dumps(rec))
        return met[:run, 3].cpu().numpy()

    fc = ec.random_case(1, O, A, H, B, mb, max(args.epochs, 300), lr=3e-4)
    call(fc, "warmup", 8, np.inf, 8, 2, timed=False)
    call(fc, "warmup", 8, np.inf, 8, 1, timed=False)
    for streams in (1, 2):
        for chunk in (1, 2, 4, 16):
            call(fc, "no_stop", args.epochs, np.inf, chunk, streams)
    # a stop after epoch 10 of 300: the first seed whose ratio_delta sets a new maximum at epoch 10
    for seed in range(2, 40):
        fs = ec.random_case(seed, O, A, H, B, mb, 300, lr=3e-3)
        rd = call(fs, "probe", 11, np.inf, 16, 2, timed=False)
        if rd[10] > 1.02 * rd[:10].max():
            break
    thr = 0.5 * (rd[10] + rd[:10].max())
    for streams in (1, 2):
        for chunk in (1, 2, 4, 8, 16):
            call(fs, "stop_at_10_of_300", 300, thr, chunk, streams)
    # context: PPO's 64-row minibatch pass and its two clip + Adam calls
    pd, cd = ec.descs(fc)
    P, C = t(fc.p0), t(fc.c0)
    gp, gc, pm, pv, cm, cv = (torch.zeros_like(x) for x in (P, C, P, P, C, C))
    hp = PpoHparams(0.2, 0.0, 0.5, 0.5, 0.9, 0.999, 1e-8)
    data = [t(x).view(64, 128, -1).squeeze(-1).contiguous() for x in (fc.states, fc.actions, fc.log_probs, fc.returns, fc.advantages)]
    rows, met = t(fc.idx[0], np.int32), torch.zeros(10, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(60):
        if it == 10:
            torch.cuda.synchronize()
            e0.record()
        ctx.ppo_minibatch_fwd_bwd(pd, P, gp, cd, C, gc, met, *data, rows, hp)
        ctx.clip_adam_step(P, gp, pm, pv, it + 1, 3e-4, 0.5)
        ctx.clip_adam_step(C, gc, cm, cv, it + 1, 3e-4, 0.5)
    e1.record()
    torch.cuda.synchronize()
    rec = dict(what="ppo_minibatch_64_rows_plus_two_clip_adam", us=round(e0.elapsed_time(e1) * 1e3 / 50, 2))
    plan.append(rec)
    print(json.dumps(rec))
    if args.plan:
        os.makedirs(os.path.dirname(os.path.abspath(args.plan)), exist_ok=True)
        json.dump(plan, open(args.plan, "w"))


if __name__ == "__main__":
    main()
