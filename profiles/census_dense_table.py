"""The table of profiles/census_dense_trace.sh's output directory: per geometry, the pair per call under each
setting (wall clock, plain runs) and the cost kernels per launch (kernel trace, profiled runs), each as the median of the
three runs' medians with their range; then census on the dense plan against census on the lists with the larger spread
(a difference counts beyond three times it).

usage: python3 profiles/census_dense_table.py OUTDIR
       python3 profiles/census_dense_table.py --kernels KERNEL_TRACE.csv    one trace -> {kernel: [median ms per launch, launches]}"""
import csv
import json
import os
import sys

import numpy as np

KERNELS = ("twoview_strip_census_kernel", "twoview_rows_census_kernel", "twoview_strip_sad_kernel", "twoview_strip_cost_kernel",
           "twoview_rows_cost_kernel", "twoview_scan_kernel", "twoview_tscan_kernel", "padded_raster_kernel", "census_kernel")
SETTINGS = ("ncc", "sad_dense", "census_lists", "census_dense")


def kernel_medians(path):
    dur = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            for k in KERNELS:
                if "srh::" + k + "<" in name or "srh::" + k + "(" in name:
                    dur.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    return {k: [float(np.median(v)), len(v)] for k, v in dur.items()}


def three(values):
    return float(np.median(values)), float(min(values)), float(max(values))


def main(out):
    rows = {}
    for geo in ("c3", "c5"):
        pairs = [json.load(open(os.path.join(out, "pair_%s_%d.json" % (geo, k)))) for k in (1, 2, 3)]
        traces = [json.load(open(os.path.join(out, "kernels_%s_%d.json" % (geo, k)))) for k in (1, 2, 3)]
        print("%s, 1920x1080x256, geodesic r = 5: median of three medians [min .. max], ms; dense plan taken: %s"
              % (geo.upper(), pairs[0]["used_dense_path"]))
        for s in SETTINGS:
            rows[geo, s] = three([p["%s_ms" % s] for p in pairs])
            print("  pair per call, %-13s %8.3f [%8.3f .. %8.3f]" % ((s,) + rows[geo, s]))
        for k in KERNELS:
            if all(k in t for t in traces):
                rows[geo, k] = three([t[k][0] for t in traces])
                print("  %-28s %8.3f [%8.3f .. %8.3f] per launch, %d launches per run" % ((k,) + rows[geo, k] + (traces[0][k][1],)))
    for geo in ("c3", "c5"):
        for a, b, what in (("census_dense", "census_lists", "pair per call"),
                           ("twoview_strip_census_kernel", "twoview_rows_census_kernel", "cost kernel per launch")):
            if (geo, a) in rows and (geo, b) in rows:
                ma, la, ha = rows[geo, a]
                mb, lb, hb = rows[geo, b]
                spread = max(ha - la, hb - lb)
                verdict = "faster" if mb - ma > 3 * spread else ("slower" if ma - mb > 3 * spread else "unmoved (within three times the larger spread)")
                print("%s %s: census dense %.3f ms, census lists %.3f ms, difference %+.3f ms, larger spread %.3f ms: dense is %s"
                      % (geo.upper(), what, ma, mb, ma - mb, spread, verdict))


if __name__ == "__main__":
    if sys.argv[1] == "--kernels":
        print(json.dumps(kernel_medians(sys.argv[2])))
    else:
        main(sys.argv[1])
