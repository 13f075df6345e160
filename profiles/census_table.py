"""The table of profiles/census_trace.sh's output directory: per geometry, the pair per call under each cost
(wall clock, plain runs) and the cost kernels per launch (kernel trace, profiled runs), each as the median of the three
runs' medians with their range; then census against SAD with the larger spread.

usage: python3 profiles/census_table.py OUTDIR"""
import csv
import json
import os
import sys

import numpy as np

KERNELS = ("twoview_rows_sad_kernel", "twoview_rows_census_kernel", "twoview_rows_cost_kernel", "twoview_strip_cost_kernel",
           "census_kernel")


def kernel_medians(path):
    """{kernel: (median ms per launch, launches)} of one kernel trace"""
    dur = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            for k in KERNELS:
                if "srh::" + k + "<" in name or "srh::" + k + "(" in name:
                    dur.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    return {k: (float(np.median(v)), len(v)) for k, v in dur.items()}


def three(values):
    """median of the three medians, their range"""
    return float(np.median(values)), float(min(values)), float(max(values))


def main(out):
    rows = {}
    for geo in ("c3", "c5"):
        pairs = [json.load(open(os.path.join(out, "pair_%s_%d.json" % (geo, k)))) for k in (1, 2, 3)]
        traces = [kernel_medians(os.path.join(out, "kernel_trace_%s_%d.csv" % (geo, k))) for k in (1, 2, 3)]
        print("%s, 1920x1080x256, geodesic r = 5: median of three medians [min .. max], ms" % geo.upper())
        for cost in ("ncc", "sad", "census"):
            rows[geo, cost] = three([p["%s_ms" % cost] for p in pairs])
            print("  pair per call, %-6s  %8.3f [%8.3f .. %8.3f]" % ((cost,) + rows[geo, cost]))
        for k in KERNELS:
            if all(k in t for t in traces):
                rows[geo, k] = three([t[k][0] for t in traces])
                print("  %-28s %8.3f [%8.3f .. %8.3f] per launch, %d launches per run" % ((k,) + rows[geo, k] + (traces[0][k][1],)))
    for geo in ("c3", "c5"):
        for a, b, what in (("census", "sad", "pair per call"), ("twoview_rows_census_kernel", "twoview_rows_sad_kernel", "rows kernel per launch")):
            if (geo, a) in rows and (geo, b) in rows:
                ma, la, ha = rows[geo, a]
                mb, lb, hb = rows[geo, b]
                spread = max(ha - la, hb - lb)
                verdict = "faster" if mb - ma > 3 * spread else ("slower" if ma - mb > 3 * spread else "within three times the larger spread")
                print("%s %s: census %.3f ms, SAD %.3f ms, difference %+.3f ms, larger spread %.3f ms: census is %s"
                      % (geo.upper(), what, ma, mb, ma - mb, spread, verdict))


if __name__ == "__main__":
    main(sys.argv[1])
