#!/bin/bash
# profiles/sad_trace.sh -- kernel trace of the SAD matching cost against NCC at 1920x1080x256: C3 and C5,
# both costs, through profiles/sad_pair.py.  usage (from the repo root, on an MI355X): bash profiles/sad_trace.sh OUTDIR
set -u
OUT=${1:?usage: bash profiles/sad_trace.sh OUTDIR}
mkdir -p "$OUT"
timeout -k 10 300 python3 profiles/sad_pair.py 3 > "$OUT/sad_pair.json" 2> "$OUT/sad_pair.err" || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/stats_sad" --output-format csv -- python3 profiles/sad_pair.py 1 \
	> "$OUT/stats_sad.log" 2>&1 || exit $?
cp "$(find "$OUT/stats_sad" -name '*kernel_stats.csv' | head -1)" "$OUT/sad_kernel_stats.csv"
cp "$(find "$OUT/stats_sad" -name '*kernel_trace.csv' | head -1)" "$OUT/sad_kernel_trace.csv"
rm -rf "$OUT/stats_sad"
