#!/bin/bash
# rocprofv3 kernel statistics of a short bench run (2 timed steps + 1 warmup, 2 C=1 queries).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT/prof_final
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_final -o run -- python3 bench.py --steps 2 --warmup 1 --full --c1 2 --c1-tp 0 > $OUT/prof_final.log 2>&1 || exit $?
s=$(find $OUT/prof_final -name "*kernel_stats.csv" | head -1)
python tools/rocprof_summary.py "$s" 40 > $OUT/prof_final_summary.txt && head -24 $OUT/prof_final_summary.txt
f=$(find $OUT/prof_final -name "*kernel_trace.csv" | head -1)
rm -f "$f"
