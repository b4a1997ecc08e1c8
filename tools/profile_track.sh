#!/bin/bash
# kernel-trace profile of the tracking loop (tools/bench_track.py), per mode -> $OUT/kernel_stats_trk_*.txt (OUT defaults to bench_out/)
export TMPDIR=/tmp
cd "$(dirname "${BASH_SOURCE[0]}")/.." || exit 1
OUT="${OUT:-bench_out}"; mkdir -p "$OUT"
for m in WB B2A; do
  rm -rf "$OUT/prof_trk_$m"
  ep=100; [ $m = B2A ] && ep=1000
  timeout 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_trk_$m" -o t -- python tools/bench_track.py --mode $m --epochs $ep > "$OUT/prof_trk_$m.log" 2>&1
  rc=$?
  tail -1 "$OUT/prof_trk_$m.log" | cut -c1-300
  python tools/rocprof_summary.py $(find "$OUT/prof_trk_$m" -name "*_results.db" | head -1) > "$OUT/kernel_stats_trk_$m.txt"
  head -6 "$OUT/kernel_stats_trk_$m.txt"
  find "$OUT/prof_trk_$m" -name "*.db" -size +20M -delete
  case $rc in 124|134|137|139) echo "$m rc=$rc"; exit $rc ;; esac  # time limit, abort or fault: nothing more on the GPU
done
