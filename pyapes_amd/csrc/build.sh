#!/bin/bash
# Build libpyapes_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   -ffp-contract=off : the stencil arithmetic must round every product and sum
#                       separately to reproduce the reference bit for bit (pa_device.h)
# The translation units are compiled in parallel (objects under build/, git-ignored), then linked.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
OBJ="$HERE/build"
mkdir -p "$OUT" "$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-variable ${PA_EXTRA_FLAGS:-})
TUS=(pa_core pa_bc pa_ops pa_march pa_project pa_stats pa_solver pa_cg pa_bicgstab pa_jacobi pa_cg3d pa_cg3d_b pa_sf pa_sf_self pa_sf_src pa_sf_src_bcl pa_sf_vel pa_sf_vself pa_sfq pa_sfq_src pa_sft pa_sfn pa_comm pa_rfp pa_resident pa_place)
pids=()
objs=()
for tu in "${TUS[@]}"; do
  "$HIPCC" "${FLAGS[@]}" -c "$HERE/$tu.hip" -o "$OBJ/$tu.o" &
  pids+=($!)
  objs+=("$OBJ/$tu.o")
done
for p in "${pids[@]}"; do wait "$p"; done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT/libpyapes_hip.so" "${objs[@]}" -ldl
echo "built $OUT/libpyapes_hip.so"
# TEST-ONLY: the stand-in for librccl that lets the multi-rank tests run their ranks as processes sharing one GPU
# (tests/lib/pa_hostring.hip; handed to the library through pa_comm_use_impl(path), never linked into it)
TLIB="$HERE/../../tests/lib"
if [ -f "$TLIB/pa_hostring.hip" ]; then
  "$HIPCC" "${FLAGS[@]}" -shared -Wl,-Bsymbolic -o "$TLIB/libpa_hostring.so" "$TLIB/pa_hostring.hip" -lrt -lpthread
  echo "built $TLIB/libpa_hostring.so"
fi
