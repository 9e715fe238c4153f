// kernels_batch.hip -- batch proposals (gpx_sweep_batch): nb greedy picks on the live sweep cache, each conditioned on the ones
// before it at their posterior mean (Kriging believer / GP-BUCB hallucination: the mean stays, the variance shrinks).
//
// With q' a scratch copy of the cache's q_n = |V(z_n)|^2, round j scores val_n = acq(bias + p_n, max(rho - q'_n, 1e-100)), picks
// i_j = argmax over the candidates not picked yet (value descending, index ascending, NaN last: the top-k's order) and, unless
// it was the last pick, conditions on x = z_{i_j}:
//     c_n = k(x, z_n) - sum_i w_i k(x_i, z_n) - sum_{l<j} v_l[i_j] v_l[n]     w = K^-1 k(X, x)    d^2 = s2_{i_j} + sn2
//     v_j[n] = c_n / d        q'_n += v_j[n]^2
// The first two terms over d are one pass of the cache correction's rank-1 kernel (k_sweep_rankq<1> with `vout`, weight row
// [w, -1, 0..], xlast = x scaled) -- launched by the driver in api.hip between the two kernels here:
//   k_batch_pick   one workgroup: merges the per-block argmax partials, records the pick, gathers z_{i_j} (raw for k(X, x),
//                  scaled for xlast), the cross terms v_l[i_j] and 1/d, all in device scratch: the host never sees an index
//   k_batch_score  one pass over the candidates: folds the raw row into v_j and q' (round 0: q' <- q), the next round's values,
//                  and a per-block argmax partial
// The argmax runs over a total order and every candidate's arithmetic is its own thread's: results do not depend on the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpx_internal.h"
#include "gpx_math.h"

namespace gpx {

#define GPX_NEG_INF (-__builtin_huge_val())
#define GPX_IDX_NONE ((int64_t)0x7fffffffffffffffLL)

__device__ __forceinline__ bool batch_better(double av, int64_t ai, double bv, int64_t bi) {
    return (av > bv) || (av == bv && ai < bi);
}

// argmax of (v, i) over a workgroup of four 64-lane waves; the result is broadcast to every thread
__device__ __forceinline__ void batch_block_argmax(double& v, int64_t& i, double* sv, int64_t* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int64_t oi = __shfl_xor((long long)i, off);
        if (batch_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww)
        if (batch_better(sv[ww], si[ww], v, i)) { v = sv[ww]; i = si[ww]; }
}

// j < 0: round 0, q' <- q of the cache.  j >= 0: row j of V holds the rank-1 pass's (k(x, z_n) - w . k(X, z_n)) / d; the cross
// terms are taken off it in pick order, each product rounded before it is added (no contraction), then divided once by d.
__global__ __launch_bounds__(256) void k_batch_score(int j, int64_t M, const double* __restrict__ cq,
                                                     const double* __restrict__ cp, double* __restrict__ qp,
                                                     double* __restrict__ V, const double* __restrict__ cross,
                                                     const double* __restrict__ scal,
                                                     const unsigned char* __restrict__ taken, double rho, double bias,
                                                     int acq_id, double p0, double* __restrict__ s2_out,
                                                     double* __restrict__ partv, int64_t* __restrict__ parti) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double bv = GPX_NEG_INF;
    int64_t bi = GPX_IDX_NONE;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < M; n += stride) {
        double q;
        if (j < 0) {
            q = cq[n];
        } else {
#pragma clang fp contract(off)
            const double invd = scal[1];
            double t = 0.0;
            for (int l = 0; l < j; ++l) {
                const double prod = cross[l] * V[(int64_t)l * M + n];
                t = t + prod;
            }
            const double td = t * invd;
            const double v = V[(int64_t)j * M + n] - td;
            V[(int64_t)j * M + n] = v;
            const double vv = v * v;
            q = qp[n] + vv;
        }
        qp[n] = q;
        const double mu = bias + cp[n];
        const double s2 = fmax(rho - q, 1e-100);
        if (s2_out) s2_out[n] = s2;
        if (!taken[n]) {
            double val = acq_value(acq_id, mu, s2, p0);
            if (val != val) val = GPX_NEG_INF;
            if (batch_better(val, n, bv, bi)) { bv = val; bi = n; }
        }
    }
    batch_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        partv[blockIdx.x] = bv;
        parti[blockIdx.x] = bi;
    }
}

// scal: [0] d  [1] 1/d  [2] 0 (the `a` slot of launch_pend_store: no value exists)  [3] d^2
__global__ __launch_bounds__(256) void k_batch_pick(int j, int nblk, const double* __restrict__ partv,
                                                    const int64_t* __restrict__ parti, int64_t M, int d,
                                                    const double* __restrict__ Z, const double* __restrict__ invell,
                                                    const double* __restrict__ qp, const double* __restrict__ V, double rho,
                                                    double sn2, double* __restrict__ x, double* __restrict__ xs,
                                                    double* __restrict__ scal, double* __restrict__ cross,
                                                    double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                    double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double bv = GPX_NEG_INF;
    int64_t bi = GPX_IDX_NONE;
    for (int e = threadIdx.x; e < nblk; e += 256) {
        const int64_t idx = parti[e];
        if (idx != GPX_IDX_NONE && batch_better(partv[e], idx, bv, bi)) { bv = partv[e]; bi = idx; }
    }
    batch_block_argmax(bv, bi, sv, si);
    const bool none = (bi == GPX_IDX_NONE) || bi < 0 || bi >= M;      // (cannot happen while nb <= M; never index with it)
    const int64_t row = none ? 0 : bi;
    const int t = threadIdx.x;
    if (t == 0) {
        const double s2 = fmax(rho - qp[row], 1e-100);
        const double d2 = s2 + sn2;
        const double dd = sqrt(d2);
        sel_val[j] = bv;
        sel_idx[j] = none ? -1 : bi;
        sel_s2[j] = s2;
        scal[0] = dd;
        scal[1] = 1.0 / dd;
        scal[2] = 0.0;
        scal[3] = d2;
        if (!none) taken[row] = 1;
    }
    if (t < j) cross[t] = V[(int64_t)t * M + row];
    for (int k = t; k < d; k += 256) {
        const double xv = Z[row * d + k];
        x[k] = xv;
        xs[k] = xv * invell[k];
    }
}

int batch_blocks(int64_t M) {
    const int64_t b = (M + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

void launch_batch_score(hipStream_t s, int j, int64_t M, const double* cq, const double* cp, double* qp, double* V,
                        const double* cross, const double* scal, const unsigned char* taken, double rho, double bias,
                        int acq_id, double p0, double* s2_out, double* partv, int64_t* parti) {
    hipLaunchKernelGGL(k_batch_score, dim3((unsigned)batch_blocks(M)), dim3(256), 0, s, j, M, cq, cp, qp, V, cross, scal,
                       taken, rho, bias, acq_id, p0, s2_out, partv, parti);
}

void launch_batch_pick(hipStream_t s, int j, int64_t M, int d, const double* partv, const int64_t* parti, const double* Z,
                       const double* invell, const double* qp, const double* V, double rho, double sn2, double* x,
                       double* xs, double* scal, double* cross, double* sel_val, int64_t* sel_idx, double* sel_s2,
                       unsigned char* taken) {
    hipLaunchKernelGGL(k_batch_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), partv, parti, M, d, Z, invell, qp, V,
                       rho, sn2, x, xs, scal, cross, sel_val, sel_idx, sel_s2, taken);
}

}  // namespace gpx
