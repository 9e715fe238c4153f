#!/bin/bash
# the stand-alone A/B binary of the sweep schedules: the library's kernels_sweep.hip is compiled INTO it
# (kernels_bound32.hip beside it: kernels_sweep.hip's bound pass calls its launcher; the probe never runs it)
cd "$(dirname "$0")" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value -DGPX_SWEEP_PROBES -I../../include -o sweep_ab.bin sweep_ab.hip ../../pybo_amd/csrc/kernels_bound32.hip
