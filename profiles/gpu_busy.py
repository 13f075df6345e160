#!/usr/bin/env python3
"""GPU busy time from a rocprofv3 --kernel-trace CSV: the union of the kernels' [start, end) intervals against the span
from the first start to the last end of a region of the trace, the largest gaps and what follows them.

  gpu_busy.py kernel_trace.csv                      the whole trace
  gpu_busy.py kernel_trace.csv NAME I J             from the dispatch after the I-th to the J-th dispatch (1-based) of
                                                    the kernel whose name contains NAME -- e.g. `mvs_cross_check 16 24`
                                                    is the third step of a C4 run (8 cross-checks end a step).  A bench.py
                                                    run ends in untimed passes (per-kernel durations, recounts): "the last N
                                                    dispatches" is not the timed region.
  gpu_busy.py --timeline kernel_trace.csv [NAME I J]  and every dispatch of the region: start and end in microseconds after
                                                    the region's first dispatch, its stream (the trace's Stream_Id, else its
                                                    Queue_Id), workgroups, and how many other dispatches run during it; then the
                                                    time the device runs nothing but dispatches of at most SMALL workgroups
"""
import csv
import sys

SMALL = 8            # workgroups: a dispatch this small leaves the device all but empty

argv = sys.argv[1:]
timeline = bool(argv) and argv[0] == "--timeline"
if timeline:
    argv = argv[1:]
rows = list(csv.DictReader(open(argv[0])))


def stream_of(r):
    return r.get("Stream_Id") or r.get("Queue_Id") or "?"


def workgroups(r):
    n = 1
    for ax in "XYZ":
        g, w = int(r.get("Grid_Size_" + ax) or 1), int(r.get("Workgroup_Size_" + ax) or 1)
        n *= max(1, (g + w - 1)//max(1, w))
    return n


ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0][-60:], stream_of(r), workgroups(r))
            for r in rows)
if len(argv) > 3:
    hits = [i for i, e in enumerate(ev) if argv[1] in e[2]]
    ev = ev[hits[int(argv[2]) - 1] + 1: hits[int(argv[3]) - 1] + 1]
t0 = ev[0][0]
span = max(e[1] for e in ev) - t0
busy, cur, gaps = 0, t0, []
for s, e, n, _, _ in ev:
    if s > cur:
        gaps.append((s - cur, n))
    busy += max(0, e - max(s, cur))
    cur = max(cur, e)
print(f"dispatches {len(ev)}  span {span/1e6:.3f} ms  busy {busy/1e6:.3f} ms ({100*busy/span:.1f} %)  "
      f"idle {(span-busy)/1e6:.3f} ms in {len(gaps)} gaps")
for g, n in sorted(gaps, reverse=True)[:10]:
    print(f"  gap {g/1e3:8.1f} us  before {n}")

if timeline:
    print(f"{'start us':>10} {'end us':>10} {'us':>9}  {'stream':>6} {'wgs':>7} {'beside':>6}  kernel")
    for s, e, n, st, wg in ev:
        beside = sum(1 for s2, e2, *_ in ev if s2 < e and e2 > s) - 1
        print(f"{(s-t0)/1e3:10.1f} {(e-t0)/1e3:10.1f} {(e-s)/1e3:9.1f}  {st:>6} {wg:7d} {beside:6d}  {n}")
    # the time during which something runs and everything that runs is a small dispatch
    cuts = sorted({t for s, e, *_ in ev for t in (s, e)})
    small_only = 0
    for a, b in zip(cuts, cuts[1:]):
        live = [wg for s, e, _, _, wg in ev if s <= a and e >= b]
        if live and max(live) <= SMALL:
            small_only += b - a
    print(f"only dispatches of <= {SMALL} workgroups running: {small_only/1e3:.1f} us of {span/1e3:.1f} us")
