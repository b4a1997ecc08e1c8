#!/bin/bash
# Measurement pass (GPU box): default bench lines, kernel-trace stats (cfg3, cfg2, tracking), PMC counters of the N-point pair.
# Everything lands under $OUT (default bench_out/); tools/collect_pass.sh PREFIX copies the summaries into profiles/ afterwards.
# A step that ends on a time limit, an abort or a fault (status 124, 134, 137, 139) ends the pass there.
export TMPDIR=/tmp
cd "$(dirname "${BASH_SOURCE[0]}")/.." || exit 1
export OUT="${OUT:-bench_out}"; mkdir -p "$OUT"  # (the scripts below write there too)
check() {  # status, step name
    echo "$2 rc=$1"
    case $1 in 124|134|137|139) echo "$2 ended on a time limit, abort or fault: nothing more is started"; exit "$1" ;; esac
}
timeout -k 10 1200 python bench.py --full > "$OUT/bench_b1c.json" 2> "$OUT/bench_b1c.err"; check $? "bench b1c"
timeout -k 10 600 python bench.py --full --workload b2a > "$OUT/bench_b2a.json" 2> "$OUT/bench_b2a.err"; check $? "bench b2a"
bash tools/profile_run.sh > "$OUT/profile_run.log" 2>&1; rc=$?; tail -3 "$OUT/profile_run.log"; check $rc profile_run
bash tools/profile_track.sh > "$OUT/profile_track.log" 2>&1; rc=$?; tail -3 "$OUT/profile_track.log"; check $rc profile_track
# (8 PRNs = one launch pair of the library default: 1608 cells; PMC_CELLS of tools/collect_pass.sh says the same)
BENCH_ARGS="--workload b1c --steps 1 --warmup 0 --no-cpu-baseline --no-tracking --no-strict-f32 --no-b2a --no-cold --prns 8" bash tools/pmc_run.sh > "$OUT/pmc_run.log" 2>&1
rc=$?; tail -2 "$OUT/pmc_run.log"; check $rc pmc_run
cp "$OUT/pmc_summary.txt" "$OUT/pmc_summary_default.txt"
