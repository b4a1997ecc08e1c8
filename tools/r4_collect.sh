#!/bin/bash
# copy the summaries of a tools/r4_profile.sh pass from gpurun_out/ into profiles/ (run here, after the gpurun call) and rebuild
# the derived files (traffic_b1c.json, valu_b1c.json)
cd "$(dirname "${BASH_SOURCE[0]}")/.."
cp gpurun_out/kernel_stats_b1c.txt profiles/r04_b1c_kernel_stats.txt
cp gpurun_out/kernel_stats_b2a.txt profiles/r04_b2a_kernel_stats.txt
cp gpurun_out/kernel_stats_trk_B2A.txt profiles/r04_trk_b2a_kernel_stats.txt
cp gpurun_out/kernel_stats_trk_WB.txt profiles/r04_trk_wb_kernel_stats.txt
cp gpurun_out/r04_phases.txt profiles/r04_phases.txt
cp gpurun_out/r04_coissue.txt profiles/r04_coissue.txt
cp gpurun_out/r04_sieve_error.txt profiles/r04_sieve_error.txt
cp gpurun_out/r04_plan_729.txt profiles/r04_plan_729.txt
grep -o "Power (W): [0-9.]*\|sclk clock level: [0-9S]: ([0-9]*Mhz)" gpurun_out/r04_power_samples.txt | paste - - > profiles/r04_power_samples.txt
tail -1 "${BENCH_OUT:-bench_out}/bench_b1c.json" > profiles/r04_bench_b1c.json
tail -1 "${BENCH_OUT:-bench_out}/bench_b2a.json" > profiles/r04_bench_b2a.json
cp gpurun_out/bench_under_rocprof_b1c.json profiles/r04_bench_b1c_under_rocprof.json 2>/dev/null
python tools/make_traffic.py gpurun_out/pmc_summary_default.txt b1c 201 profiles/r04_b1c_pmc.txt k_cols_wave_f "round 4" > /dev/null
python tools/make_valu.py gpurun_out/pmc_summary_default.txt profiles/r04_isa_mix.json b1c 201 "round 4" > /dev/null
python - <<'PY'
import json
j = json.load(open("profiles/r04_bench_b1c.json")); r = j["roofline"]; v = r.get("valu") or {}
print("b1c: ms/step %.1f frac %.3f pair %.3f rows %.3f cols %.3f clock %s" % (j["ms_per_step"], r["frac"], r["pair_ms"], r["rows_ms"], r["cols_ms"], v.get("shader_clock_GHz")))
print("b2a key:", j.get("b2a", {}).get("ms_per_step"), (j.get("b2a") or {}).get("stage_ms"))
t = json.load(open("profiles/traffic_b1c.json")); print("traffic GB/pair %.2f" % (t["bytes_per_pair"] / 1e9))
u = json.load(open("profiles/valu_b1c.json")); print("bound ms %.3f additive %.3f" % (u["bound_ms"], u["additive_r3_bound_ms"]), {k: round(x["valu_busy"] or 0, 3) for k, x in u["kernels"].items()})
PY
