#!/usr/bin/env python
"""Rollout section of a rocprofv3 kernel trace (rocpd sqlite) of bench.py: per rollout, the acting launches (k_rollout_step /
k_rollout_steps) on the main stream and the permutation prefetch's kernels (k_random_bits, k_tile_iota, k_rs_*) on the side
stream -- does the side stream's chain still run UNDER the acting launches, i.e. does its last kernel end before the last
acting launch does?  (k_rs_scatter needs 36 KB of LDS next to a resident acting workgroup.)
Usage: python tools/rollout_timeline.py <results.db> [rollouts to print, default 3]"""
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
name_col = "name" if "name" in cols else "kernel_name"
rows = cur.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
acting = [(s, e) for n, s, e in rows if "k_rollout_step" in n]
perm = [(n, s, e) for n, s, e in rows if any(k in n for k in ("k_rs_", "k_tile_iota", "k_random_bits"))]
groups, curg = [], []
for s, e in acting:                      # a rollout = acting launches less than 5 ms apart (the update between two takes ~56 ms)
    if curg and s - curg[-1][1] > 5e6:
        groups.append(curg)
        curg = []
    curg.append((s, e))
if curg:
    groups.append(curg)
print(f"{len(groups)} rollouts, {len(acting)} acting launches, {len(perm)} permutation-prefetch kernels in the trace")
print("rollout  launches  span_us  busy_us | perm kernels  first_start_us  last_end_us  scatter_inside | margin_us (last acting end - last perm end)")
for gi, g in list(enumerate(groups))[-int(sys.argv[2]) if len(sys.argv) > 2 else -3:]:
    t0, t1 = g[0][0], g[-1][1]
    busy = sum(e - s for s, e in g)
    pk = [(n, s, e) for n, s, e in perm if s >= t0 - 2e6 and s <= t1 + 5e6]
    if not pk:
        print(f"{gi:7d} {len(g):9d} {(t1 - t0) / 1e3:8.1f} {busy / 1e3:8.1f} | none")
        continue
    last_end = max(e for _, _, e in pk)
    inside = sum(1 for n, s, e in pk if "k_rs_scatter" in n and any(a <= s and e <= b for a, b in g))
    nsc = sum(1 for n, _, _ in pk if "k_rs_scatter" in n)
    print(f"{gi:7d} {len(g):9d} {(t1 - t0) / 1e3:8.1f} {busy / 1e3:8.1f} | {len(pk):12d} {(min(s for _, s, _ in pk) - t0) / 1e3:15.1f} "
          f"{(last_end - t0) / 1e3:12.1f} {inside:8d}/{nsc:<5d} | {(t1 - last_end) / 1e3:9.1f}")
