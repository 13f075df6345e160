#!/bin/bash
# profiles/sad_dense_trace.sh -- the SAD matching cost of the C3 pair on the dense plan against the row-run lists
#  through profiles/sad_dense_pair.py: the pair time three times over with the two passes side by side,
# three times with one after the other, then one kernel trace of the same script (with a few NCC pairs behind, for the
# NCC strip kernel).  usage (from the repo root, on an MI355X): bash profiles/sad_dense_trace.sh OUTDIR
set -u
OUT=${1:?usage: bash profiles/sad_dense_trace.sh OUTDIR}
mkdir -p "$OUT"
: > "$OUT/sad_dense_pair.json"
for k in 1 2 3; do
	timeout -k 10 200 python3 profiles/sad_dense_pair.py 20 1 >> "$OUT/sad_dense_pair.json" 2>> "$OUT/sad_dense_pair.err" || exit $?
done
for k in 1 2 3; do
	timeout -k 10 200 python3 profiles/sad_dense_pair.py 20 0 >> "$OUT/sad_dense_pair.json" 2>> "$OUT/sad_dense_pair.err" || exit $?
done
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/stats_sad_dense" --output-format csv -- python3 profiles/sad_dense_pair.py 8 0 1 \
	> "$OUT/stats_sad_dense.log" 2>&1 || exit $?
cp "$(find "$OUT/stats_sad_dense" -name '*kernel_stats.csv' | head -1)" "$OUT/sad_dense_kernel_stats.csv"
rm -rf "$OUT/stats_sad_dense"
