#!/bin/bash
# copy the summaries of a tools/measure_pass.sh pass from $OUT (default bench_out/) into profiles/ (run here, after the GPU call)
# and rebuild the derived files (traffic_b1c.json, valu_b1c.json) for the N-point pair
#   tools/collect_pass.sh PREFIX [LABEL]   e.g. tools/collect_pass.sh r07 "round 7" -> profiles/r07_*
# make_valu.py prices the kernels from profiles/PREFIX_isa_mix.json (tools/isa_mix.py ... pfa), which must exist.
[ -n "$1" ] || { echo "usage: $0 PREFIX [LABEL]" >&2; exit 2; }
P="$1"; LABEL="${2:-$1}"
cd "$(dirname "${BASH_SOURCE[0]}")/.."
OUT="${OUT:-bench_out}"
cp "$OUT/kernel_stats_b1c.txt" profiles/${P}_b1c_kernel_stats.txt
cp "$OUT/kernel_stats_b2a.txt" profiles/${P}_b2a_kernel_stats.txt
cp "$OUT/kernel_stats_trk_B2A.txt" profiles/${P}_trk_b2a_kernel_stats.txt
cp "$OUT/kernel_stats_trk_WB.txt" profiles/${P}_trk_wb_kernel_stats.txt
tail -1 "$OUT/bench_b1c.json" > profiles/${P}_bench_b1c.json
tail -1 "$OUT/bench_b2a.json" > profiles/${P}_bench_b2a.json
cp "$OUT/bench_under_rocprof_b1c.json" profiles/${P}_bench_b1c_under_rocprof.json 2>/dev/null
python tools/make_traffic.py "$OUT/pmc_summary_default.txt" b1c ${PMC_CELLS:-1608} profiles/${P}_b1c_pmc.txt k_pfa_cols "$LABEL" 2 > /dev/null
python tools/make_valu.py "$OUT/pmc_summary_default.txt" profiles/${P}_isa_mix.json b1c ${PMC_CELLS:-1608} "$LABEL" pfa > /dev/null
P="$P" python - <<'PY'
import json, os
p = os.environ["P"]
j = json.load(open(f"profiles/{p}_bench_b1c.json")); r = j["roofline"]; v = r.get("valu") or {}
print("b1c: ms/step %.1f frac %.3f pair %.3f rows %.3f cols %.3f clock %s" % (j["ms_per_step"], r["frac"], r["pair_ms"], r["rows_ms"], r["cols_ms"], v.get("shader_clock_GHz")))
print("b2a key:", j.get("b2a", {}).get("ms_per_step"), (j.get("b2a") or {}).get("stage_ms"))
t = json.load(open("profiles/traffic_b1c.json")); print("traffic GB/pair %.2f (%.1f MB per cell)" % (t["bytes_per_pair"] / 1e9, t["per_cell_MB"]))
u = json.load(open("profiles/valu_b1c.json")); print("bound ms %.3f" % u["bound_ms"], {k: round(x["valu_busy"] or 0, 3) for k, x in u["kernels"].items()})
PY
