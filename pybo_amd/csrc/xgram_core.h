// xgram_core.h -- the squared scaled distances of one 64 x 128 tile of a cross-Gram, shared by every kernel that forms such a tile
// on the VALU: k_cross_gram (kernels_sweep.hip: the tile goes to HBM) and k_path_update (kernels_path.hip: the tile goes to LDS
// and on to the matrix pipe).  One definition, so that k(X_i, x_m) has the same bits wherever it is formed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpx {

// tile 64 observed rows x 128 candidate columns, 8 x 4 outputs per thread (256 threads); coordinates staged XDC at a time
constexpr int XK = 64, XN = 128, XDC = 16;

// Staging of a (rows x kc) block of row-major coordinates into LDS as [k][row] WITHOUT index divisions: a thread owns
// one row and every STRIDE-th coordinate of it (counters: the e / kc, e % kc form cost ~13 of 50-58 VALU instructions
// per covariance evaluation at d = 8 -- these kernels are VALU-issue-bound).
// Squared scaled distances of an 8 x 4 block per thread, one dimension at a time; the first dimension starts the sums
// (df * df == fma(df, df, +0): same bits as a zero-initialised accumulator).
template <bool FIRST>
__device__ __forceinline__ void dist_step(const double (*xo)[XK], const double (*xc)[XN], int k, int ty, int tx,
                                          double (&r2)[8][4]) {
    double a8[8], b4[4];
#pragma unroll
    for (int a = 0; a < 8; ++a) a8[a] = xo[k][ty * 8 + a];
#pragma unroll
    for (int b = 0; b < 4; ++b) b4[b] = xc[k][tx * 4 + b];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double df = a8[a] - b4[b];
            r2[a][b] = FIRST ? df * df : fma(df, df, r2[a][b]);
        }
}

// the candidates' scaled coordinates [c0, c0 + kc) of the workgroup's 128 columns -> xc (candidate gmc >= M: zeros); the caller
// places the barriers
__device__ __forceinline__ void xgram_stage_cand(double (*xc)[XN], const double* __restrict__ Xc, int64_t gmc, int64_t M, int d,
                                                 const double* __restrict__ invell, int c0, int kc) {
    const int t = threadIdx.x, crow = t & (XN - 1), ckq = t >> 7;      // row, first coordinate (stride 2)
    for (int k = ckq; k < kc; k += 2) xc[k][crow] = (gmc < M) ? Xc[gmc * d + c0 + k] * invell[c0 + k] : 0.0;
}

// r2[a][b] = |Xs[k0 + 8 ty + a] - xc[4 tx + b]|^2 over all d coordinates of the observed rows k0 .. k0 + 63 (rows of the scaled,
// zero-padded Xs: every row read must exist) and the workgroup's 128 candidates, whose first global index is gm0.  onepass
// (d <= XDC): xc already holds the candidates (xgram_stage_cand once per workgroup); else they are staged again with every
// XDC coordinates.  All 256 threads call it; it begins and ends its staging with a barrier.
__device__ __forceinline__ void xgram_tile_r2(double (*xo)[XK], double (*xc)[XN], const double* __restrict__ Xs, int64_t k0, int d,
                                              const double* __restrict__ Xc, int64_t gm0, int64_t M,
                                              const double* __restrict__ invell, bool onepass, double (&r2)[8][4]) {
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const int orow = t & (XK - 1), okq = t >> 6;      // staging of observed rows: row, first coordinate (stride 4)
    const int64_t gmc = gm0 + (t & (XN - 1));
    auto stage = [&](int c0, int kc) {
        __syncthreads();
        for (int k = okq; k < kc; k += 4) xo[k][orow] = Xs[(k0 + orow) * d + c0 + k];
        if (!onepass) xgram_stage_cand(xc, Xc, gmc, M, d, invell, c0, kc);
        __syncthreads();
    };
    {
        const int kc = min(XDC, d);
        stage(0, kc);
        dist_step<true>(xo, xc, 0, ty, tx, r2);
#pragma unroll 1
        for (int k = 1; k < kc; ++k) dist_step<false>(xo, xc, k, ty, tx, r2);
    }
    for (int c0 = XDC; c0 < d; c0 += XDC) {
        const int kc = min(XDC, d - c0);
        stage(c0, kc);
#pragma unroll 1
        for (int k = 0; k < kc; ++k) dist_step<false>(xo, xc, k, ty, tx, r2);
    }
}

}  // namespace gpx
