#!/bin/bash
# Build libgpx.so and libgpx_diag.so for gfx950 in-tree (the .so files are git-ignored).
#   build.sh          compile the objects that are older than their inputs (incremental: development)
#   build.sh --force  compile EVERY object from source (what __graft_entry__.build() runs: the driver's build check must
#                     compile all seventeen translation units, also on a snapshot that shipped up-to-date .o files)
# The two libraries link the same objects but one: diag_flag.cpp, compiled twice (diag_flag.o, and diag_flag_diag.o with
# -DGPX_DIAGNOSTICS), decides whether gpx_set_option accepts the diagnostic knobs of gpx_diag.h.  The test-suite drives
# libgpx_diag.so (tests/conftest.py: GPX_DIAGNOSTICS=1); everything else loads libgpx.so.
# A/B builds (never shipped): EXTRA="-DGPX_PF16_COUNTED_WAIT" lets the diagonal role publish a step with its next tile's stores in flight (round 5's hand-counted s_waitcnt; 2-5 % faster up to N = 4096, see ADVICE round 5 for why it is off); EXTRA="-DGPX_BOUND32_NOFACT" makes
# the option bound_fact default to 0: the fp32 bound kernel with its sign tiles alone (profiles/bound_f32_ops_ab.md, build A).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-const-variable $EXTRA"
SRCS="kernels_fit kernels_chol_tg kernels_sweep kernels_mes kernels_kg kernels_rff kernels_path kernels_grad kernels_hyper kernels_ens kernels_ehvi kernels_batch kernels_cov comm api"
HDRS="xgram_core.h acq_core.h acq_core_dev.h ehvi_math.h bound_exp.h bound_f32.h gemm_core.h sweep_map.h gpx_internal.h ws_layout.h prune_hint.h gpx_diag.h gpx_math.h mes_math.h kg_math.h fit_tiles.h ../../include/gpx.h"
FORCE=0
[ "$1" = "--force" ] && FORCE=1
pids=()
n=0
# obj src [flags]: compile in the background when obj is missing, older than src or a header, or --force
compile() {
  local obj=$1 src=$2 stale=$FORCE
  shift 2
  [ -f $obj ] || stale=1
  for dep in $src $HDRS; do [ $dep -nt $obj ] && stale=1; done
  if [ $stale = 1 ]; then
    $HIPCC $FLAGS "$@" -c $src -o $obj &
    pids+=($!)
    n=$((n + 1))
  fi
}
OBJS=""
for f in $SRCS; do
  compile $f.o $f.hip
  OBJS="$OBJS $f.o"
done
compile kernels_bound32.o kernels_bound32.hip -fno-slp-vectorize      # (why: the file's header)
OBJS="$OBJS kernels_bound32.o"
compile diag_flag.o diag_flag.cpp -x c++                      # host code only (as HIP it would export one more symbol)
compile diag_flag_diag.o diag_flag.cpp -x c++ -DGPX_DIAGNOSTICS
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libgpx.so $OBJS diag_flag.o -ldl
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libgpx_diag.so $OBJS diag_flag_diag.o -ldl
echo "built $(pwd)/libgpx.so and libgpx_diag.so ($n of $(($(echo $SRCS | wc -w) + 3)) objects compiled)"
