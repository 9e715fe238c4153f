// acq_core_dev.h -- the device-only part of acq_core.h: what needs a workgroup.  One copy each of the arg-max reduction of the
// top-k and the batch picks, the parts of a batch pick kernel (merge_pick, pick_member, pick_gather), the frame of the batch scoring
// kernels (batch_score_frame) and the frame of the one-thread-per-candidate acquisition kernels (acq_frame).
#pragma once
#include <hip/hip_runtime.h>

#include "acq_core.h"

namespace gpx {

// argmax of (v, i) under `better` over a workgroup of four 64-lane waves; the result is broadcast to every thread
__device__ __forceinline__ void block_argmax(double& v, int64_t& i, double* sv, int64_t* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int64_t oi = __shfl_xor((long long)i, off);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww)
        if (better(sv[ww], si[ww], v, i)) { v = sv[ww]; i = si[ww]; }
}

// The front of a pick kernel (one workgroup of 256): merges the scoring pass's per-block argmax partials, records pick j
// (sel_val, sel_idx, taken) and returns the candidate row to gather from -- 0 when there was none, never the sentinel.
__device__ __forceinline__ int64_t merge_pick(int j, int nblk, const double* __restrict__ partv, const int64_t* __restrict__ parti,
                                              int64_t M, double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                              unsigned char* __restrict__ taken) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double bv = NEG_INF;
    int64_t bi = IDX_NONE;
    for (int e = threadIdx.x; e < nblk; e += 256) {
        const int64_t idx = parti[e];
        if (idx != IDX_NONE && better(partv[e], idx, bv, bi)) { bv = partv[e]; bi = idx; }
    }
    block_argmax(bv, bi, sv, si);
    const bool none = (bi == IDX_NONE) || bi < 0 || bi >= M;      // (cannot happen while nb <= M; never index with it)
    const int64_t row = none ? 0 : bi;
    if (threadIdx.x == 0) {
        sel_val[j] = bv;
        sel_idx[j] = none ? -1 : bi;
        if (!none) taken[row] = 1;
    }
    return row;
}

// Member e's part of pick j at candidate `row`, by thread t of the nt (>= j) that share it: its floored variance there (returned to every
// thread) into sel_s2[j] and pick_scalars' four words, the cross terms V[l][row] for l < j, and xs = z_row / ell.
__device__ __forceinline__ double pick_member(const BatchMember& e, int j, int64_t M, int d, const double* __restrict__ Z, int64_t row,
                                              double* __restrict__ sel_s2, int t, int nt) {
    const double s2 = s2_floored(e.rho, e.qp[row]);
    if (t == 0) {
        sel_s2[j] = s2;
        pick_scalars(s2, e.sn2, e.scal);
    }
    if (t < j) e.cross[t] = e.V[(int64_t)t * M + row];
    for (int k = t; k < d; k += nt) e.xs[k] = Z[row * d + k] * e.invell[k];
    return s2;
}

// the raw x = z_row, by the whole workgroup
__device__ __forceinline__ void pick_gather(const double* __restrict__ Z, int64_t row, int d, double* __restrict__ x) {
    for (int k = threadIdx.x; k < d; k += 256) x[k] = Z[row * d + k];
}

// The frame of a batch scoring kernel (256 threads per workgroup, any grid): every candidate, live or not, goes through fold(n) (its
// fold and its stores); the live ones -- not taken yet and, in a round forced to one row (forced >= 0), that row -- then through
// value(n, what fold returned), and their arg-max under the total order is the workgroup's partial.
template <class Fold, class Value>
__device__ __forceinline__ void batch_score_frame(int64_t M, const unsigned char* __restrict__ taken, int64_t forced, const Fold& fold,
                                                  const Value& value, double* __restrict__ partv, int64_t* __restrict__ parti) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double bv = NEG_INF;
    int64_t bi = IDX_NONE;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < M; n += stride) {
        const auto c = fold(n);
        if (taken[n] || (forced >= 0 && n != forced)) continue;
        const double val = nan_last(value(n, c));
        if (better(val, n, bv, bi)) { bv = val; bi = n; }
    }
    block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        partv[blockIdx.x] = bv;
        parti[blockIdx.x] = bi;
    }
}

// The frame of an acquisition kernel with one thread per candidate of the chunk at m0 (256 per workgroup): the candidate's sums and
// moments, the optional store of the sums (the state gpx_append's rank-1 correction keeps current: the same bits whichever
// acquisition seeds a sweep cache), then score(mu, s2), the only line in which such kernels differ.
template <class Score>
__device__ __forceinline__ void acq_frame(const double* __restrict__ Qp, const double* __restrict__ Pp, int64_t ldp, int nrb, int64_t m0,
                                          int64_t cols_valid, double rho, double bias, const Score& score,
                                          double* __restrict__ acq_out, double* __restrict__ mu_out, double* __restrict__ s2_out,
                                          double* __restrict__ qsum, double* __restrict__ psum) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= cols_valid) return;
    const CandMoments c = cand_moments(Qp, Pp, ldp, nrb, n, rho, bias);
    if (qsum) {
        qsum[m0 + n] = c.q;
        psum[m0 + n] = c.p;
    }
    const double val = score(c.mu, c.s2);
    acq_out[m0 + n] = val;
    if (mu_out) mu_out[m0 + n] = c.mu;
    if (s2_out) s2_out[m0 + n] = c.s2;
}

}  // namespace gpx
