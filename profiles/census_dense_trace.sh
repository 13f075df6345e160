#!/bin/bash
# profiles/census_dense_trace.sh -- the census matching cost on the dense plan against the candidate lists at 1920x1080x256
# (DESIGN.md 4p): C3 and C5, the settings alternating on one context through profiles/census_dense_pair.py, 20 timed calls
# each, the script three times plain for the wall clock per pair and three times under rocprofv3 --kernel-trace --stats (runs
# of their own, no counters) for the kernels' durations per launch.  profiles/census_dense_table.py OUTDIR prints the table
# of both.  A step that fails, faults or runs into its time limit ends the script.
# usage (from the repo root, on an MI355X): bash profiles/census_dense_trace.sh OUTDIR
set -u
OUT=${1:?usage: bash profiles/census_dense_trace.sh OUTDIR}
STEPS=${STEPS:-20}
mkdir -p "$OUT"
for geo in c3 c5; do
	for k in 1 2 3; do
		timeout -k 10 240 python3 profiles/census_dense_pair.py "$STEPS" "$geo" > "$OUT/pair_${geo}_$k.json" 2> "$OUT/pair_${geo}_$k.err" || exit $?
		timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/stats_${geo}_$k" --output-format csv -- python3 profiles/census_dense_pair.py "$STEPS" "$geo" \
			> "$OUT/stats_${geo}_$k.log" 2>&1 || exit $?
		f=$(find "$OUT/stats_${geo}_$k" -name "*kernel_trace.csv" | head -1)
		if [ -z "$f" ]; then echo "census_dense_trace.sh: rocprofv3 wrote no *kernel_trace.csv under $OUT/stats_${geo}_$k (see $OUT/stats_${geo}_$k.log)" >&2; exit 1; fi
		python3 profiles/census_dense_table.py --kernels "$f" > "$OUT/kernels_${geo}_$k.json" || exit $?
		rm -rf "$OUT/stats_${geo}_$k"
	done
done
python3 profiles/census_dense_table.py "$OUT" | tee "$OUT/census_dense_table.txt"
