#!/bin/bash
# Kernel-trace profiles of the default bench commands (GPU box):
#   bash tools/profile_run.sh            -> $OUT/prof_b1c, $OUT/prof_b2a + text summaries (OUT defaults to bench_out/)
export TMPDIR=/tmp
cd "$(dirname "${BASH_SOURCE[0]}")/.." || exit 1
OUT="${OUT:-bench_out}"; mkdir -p "$OUT"
for w in b1c b2a; do
  rm -rf "$OUT/prof_$w"
  timeout 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$w" -o $w -- python bench.py --workload $w --no-cpu-baseline --no-tracking --no-strict-f32 --no-b2a > "$OUT/prof_$w.log" 2>&1
  rc=$?; echo "$w rc=$rc"
  db=$(find "$OUT/prof_$w" -name "*_results.db" | head -1)
  python tools/rocprof_summary.py "$db" > "$OUT/kernel_stats_$w.txt"
  grep -E "^\{" "$OUT/prof_$w.log" > "$OUT/bench_under_rocprof_$w.json"
  find "$OUT/prof_$w" -name "*.db" -size +20M -delete
  head -8 "$OUT/kernel_stats_$w.txt"
  case $rc in 124|134|137|139) exit $rc ;; esac  # time limit, abort or fault: nothing more on the GPU
done
