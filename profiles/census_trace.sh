#!/bin/bash
# profiles/census_trace.sh -- the census matching cost against SAD and NCC at 1920x1080x256: C3 and C5, the
# three costs alternating on one context through profiles/census_pair.py, 20 timed calls each, the script three times
# over -- once plain for the wall clock per pair, once under rocprofv3 --kernel-trace --stats (a run of its own) for the
# kernels' durations per launch.  profiles/census_table.py OUTDIR prints the table of both.
# usage (from the repo root, on an MI355X): bash profiles/census_trace.sh OUTDIR
set -u
OUT=${1:?usage: bash profiles/census_trace.sh OUTDIR}
STEPS=${STEPS:-20}
mkdir -p "$OUT"
for geo in c3 c5; do
	for k in 1 2 3; do
		timeout -k 10 240 python3 profiles/census_pair.py "$STEPS" "$geo" > "$OUT/pair_${geo}_$k.json" 2> "$OUT/pair_${geo}_$k.err" || exit $?
		timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/stats_${geo}_$k" --output-format csv -- python3 profiles/census_pair.py "$STEPS" "$geo" \
			> "$OUT/stats_${geo}_$k.log" 2>&1 || exit $?
		for what in kernel_stats kernel_trace; do
			f=$(find "$OUT/stats_${geo}_$k" -name "*$what.csv" | head -1)
			if [ -z "$f" ]; then echo "census_trace.sh: rocprofv3 wrote no *$what.csv under $OUT/stats_${geo}_$k (see $OUT/stats_${geo}_$k.log)" >&2; exit 1; fi
			cp "$f" "$OUT/${what}_${geo}_$k.csv" || exit $?
		done
		rm -rf "$OUT/stats_${geo}_$k"
	done
done
python3 profiles/census_table.py "$OUT" | tee "$OUT/census_table.txt"
