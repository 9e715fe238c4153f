// kernels_ehvi.hip -- the fold of a two-objective sweep (gpx_ehvi_sweep*, gpx_ehvi_fold_dev): the expected
// hypervolume improvement of every candidate from the four posterior moments the two member sweeps left in HBM and the strips of the
// front.  ehvi_math.h holds the arithmetic (ehvi_value, ehvi_fold_term); every EI is gpx_math.h's acq_value, compiled here under the
// same default contraction as in k_acq (no file-level pragma: the empty front must return the bits of gpx_sweep(GPX_ACQ_EI)).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpx_internal.h"
#include "gpx_math.h"
#define GPX_EHVI_DEVICE
#include "ehvi_math.h"

namespace gpx {

// One thread per candidate, grid-stride.  mom (4, M): mu1, s2_1, mu2, s2_2.  strips: a[0 .. n + 1] then b[0 .. n + 1] (b[n + 1] is
// padding), 2 (n + 2) doubles, staged once per workgroup into LDS; in the loop every lane reads the same word of a and of b in the same
// iteration, which the LDS broadcasts.  A candidate's value depends on the bits of its four moments and of the strips alone: not on M,
// its position or the launch shape.  Compute-bound: 2 (n + 1) + 1 EI evaluations per candidate.
__global__ __launch_bounds__(256) void k_ehvi_fold(const double* __restrict__ mom, int64_t M, const double* __restrict__ strips, int n,
                                                   double* __restrict__ out) {
    __shared__ double sa[EHVI_STRIP_LD], sb[EHVI_STRIP_LD];
    for (int i = threadIdx.x; i < n + 2; i += blockDim.x) {
        sa[i] = strips[i];
        sb[i] = strips[n + 2 + i];
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += stride)
        out[m] = ehvi_value(mom[m], mom[M + m], mom[2 * M + m], mom[3 * M + m], sa, sb, n);
}

// (n <= EHVI_MAX_FRONT: the caller's check; the strips hold 2 (n + 2) doubles)
void launch_ehvi_fold(hipStream_t s, const double* mom, int64_t M, const double* strips, int n, double* out) {
    int64_t b = (M + 255) / 256;
    b = b < 1 ? 1 : (b > 4096 ? 4096 : b);
    hipLaunchKernelGGL(k_ehvi_fold, dim3((unsigned)b), dim3(256), 0, s, mom, M, strips, n, out);
}

}  // namespace gpx
