#!/bin/bash
# Probe build for tools/deep_timing.py --probe-lib: the library with the surface stores of the deep search's column pass compiled
# out (k_cols_deep<NC, false>, csrc/bds_acq_deep.h), so that the pass's time without its read-modify-write can be measured.  Its
# results are meaningless; nothing loads it but that tool.  Needs the objects of a finished ./build.sh.
#   bash tools/build_deep_probe.sh   -> <package>/libbds_mi355x_deep_probe.so
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
PKG="$ROOT/bds-3-b1c-b2a-sdr-receiver_amd"
BLD="$PKG/build"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
mkdir -p "$BLD/probe"
"$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-result -I"$ROOT/include" -I"$PKG/csrc" \
    -ffp-contract=fast -fno-slp-vectorize -DBDS_DEEP_PROBE_NO_STORE -c "$PKG/csrc/bds_acq.hip" -o "$BLD/probe/bds_acq.o"
objs=("$BLD/probe/bds_acq.o")
for o in "$BLD"/*.o; do
    case "$(basename "$o")" in bds_acq.o|*_hooks.o) ;; *) objs+=("$o") ;; esac
done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o "$PKG/libbds_mi355x_deep_probe.so" -ldl -Wl,-rpath,/opt/rocm/lib
echo "built $PKG/libbds_mi355x_deep_probe.so"
