// kernels_hyper.hip -- gradient of the log marginal likelihood with respect to the hyper-parameters, on a fitted handle.
//
//   Ky = K + sn2 I,  alpha = Ky^-1 (y - bias),  Kinv = Ky^-1 = T^T T  (T = R^-T, lower),  W = alpha alpha^T - Kinv
//   dL/dsn2   = 1/2 sum_i  W_ii
//   dL/drho   = 1/2 sum_ij W_ij k_ij / rho                                   (k without the noise term)
//   dL/dell_k = 1/2 sum_ij W_ij g_ij (-2 (xs_ik - xs_jk)^2 / ell_k)           (g = dk/dr2, xs = x / ell: the handle's Xs)
//   dL/dbias  = sum_i alpha_i
//
// k_loglik_grad_tiles: one workgroup per lower 128x128 tile (I, J), I >= J, of Kinv:
//     Kinv(I, J) = sum_{K >= I} T(K, I)^T T(K, J)
// Both operands are k-major views of the row-major T (A(m, k) = T[k Np + i0 + m], B(k, n) = T[k Np + j0 + n]): no transposed
// copy.  The K-extent of a tile is nP - I blocks, so the tiles are numbered by rows of I ascending: heaviest first.  Padding:
// rows k >= N of T are identity rows (zero in every real column), so they add exact zeros to the real entries; entries with
// i >= N or j >= N are masked in the epilogue.
// FUSED epilogue -- Kinv never reaches HBM.  Once the k-loop has ended its LDS holds the two blocks' rows of Xs, 32
// coordinates at a time (beyond d = 32: in slabs).  Pass 1 forms r2 for the thread's accumulator elements and replaces each
// accumulator by c = wt W g, adding wt W k to the rho sum and W_ii to the trace (wt: 2 for an off-diagonal tile and for i > j
// on a diagonal tile, 1 for i = j, 0 for i < j and for padding: the lower triangle stands for the whole matrix).  Pass 2 walks
// the coordinates again: sum_k = sum c (xs_ik - xs_jk)^2.  Every sum is reduced lanes -> wave -> workgroup in a fixed order and
// written to the tile's own slot of part[tiles][d + 2]; k_loglik_grad_reduce adds the slots in a fixed order and applies the
// natural-parameter scalings once.  No floating-point atomics anywhere: the same fit gives the same bits.
#include "gemm_core.h"
#include "gpx_internal.h"
#include "gpx_math.h"

namespace gpx {

constexpr int HY_SLAB = 32;             // coordinates of Xs staged at a time
constexpr int HY_PITCH = NB + 1;        // row pitch of a staged coordinate (odd: the transposing LDS writes spread over the banks)
constexpr int HY_RED = 2 * HY_SLAB * HY_PITCH;      // offset of the per-wave partial sums [4][HY_SLAB + 2]
static_assert(HY_RED + 4 * (HY_SLAB + 2) <= GEMM_LDS_F64, "the epilogue lives in the k-loop's LDS");

// sum over the 64 lanes (xor butterfly: the same order for every lane)
__device__ __forceinline__ double hy_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(GEMM_THREADS, 2) void k_loglik_grad_tiles(const double* __restrict__ T, int64_t Np, int nP, int64_t N,
                                                                     const double* __restrict__ Xs, int d,
                                                                     const double* __restrict__ alpha, int kid, double rho,
                                                                     double* __restrict__ part) {
    // tiles (I, J), J <= I, by rows of I ascending (row I holds I + 1 tiles of K-extent nP - I blocks: heaviest first)
    int J = blockIdx.x, I = 0;
    while (J > I) { J -= I + 1; ++I; }
    __shared__ __attribute__((aligned(16))) double smem[GEMM_LDS_F64];
    const int64_t i0 = (int64_t)I * NB, j0 = (int64_t)J * NB;
    d4 acc[4][4];
    acc_zero(acc);
    gemm_tile_128_l<32, 1, 2>(acc, T + i0, Np, T + j0, Np, I * NB, (int)Np, smem);      // ends behind a barrier: the LDS is free

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double* xi = smem;                              // [HY_SLAB][HY_PITCH] coordinates of block I's rows
    double* xj = smem + HY_SLAB * HY_PITCH;         // ... of block J's
    double* red = smem + HY_RED;                    // [4][HY_SLAB + 2]
    const int nslab = (d + HY_SLAB - 1) / HY_SLAB;
    auto stage = [&](int k0, int kc) {
        for (int e = t; e < NB * kc; e += GEMM_THREADS) {
            const int row = e / kc, k = e - row * kc;
            xi[k * HY_PITCH + row] = Xs[(i0 + row) * d + k0 + k];
            xj[k * HY_PITCH + row] = Xs[(j0 + row) * d + k0 + k];
        }
    };
    int colv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) colv[j] = acc_col(j);
    double aj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) aj[j] = alpha[j0 + colv[j]];

    // ---- pass 1, one of the thread's four row blocks at a time (16 elements: r2 stays in 16 registers beside the 128 of the
    //      accumulators): r2, then c = wt W g in place of Kinv; the trace and the rho sum
    double s_tr = 0.0, s_rho = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d4 r2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r2[j] = (d4){0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < nslab; ++s) {
            const int k0 = s * HY_SLAB, kc = min(HY_SLAB, d - k0);
            if (nslab > 1 || i == 0) {              // a single slab is staged once and stays
                __syncthreads();
                stage(k0, kc);
                __syncthreads();
            }
            for (int k = 0; k < kc; ++k) {
                double b4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b4[j] = xj[k * HY_PITCH + colv[j]];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double a = xi[k * HY_PITCH + acc_row(i, r)];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double df = a - b4[j];
                        r2[j][r] = fma(df, df, r2[j][r]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = i0 + acc_row(i, r);
            const double ai = alpha[gi];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t gj = j0 + colv[j];
                const double wt = (gi < N && gj < N) ? ((I != J || gi > gj) ? 2.0 : ((gi == gj) ? 1.0 : 0.0)) : 0.0;
                const double wv = fma(ai, aj[j], -acc[i][j][r]);
                double kv, gv;
                kern_and_grad(kid, r2[j][r], rho, kv, gv);
                const bool on = wt != 0.0;
                s_rho += on ? wt * (wv * kv) : 0.0;
                s_tr += (on && gi == gj) ? wv : 0.0;
                acc[i][j][r] = on ? wt * (wv * gv) : 0.0;
            }
        }
    }
    s_tr = hy_wave_sum(s_tr);
    s_rho = hy_wave_sum(s_rho);
    if (lane == 0) {
        red[w * (HY_SLAB + 2) + HY_SLAB] = s_tr;
        red[w * (HY_SLAB + 2) + HY_SLAB + 1] = s_rho;
    }

    // ---- pass 2: per coordinate, sum c (xs_ik - xs_jk)^2   (a single slab is still in LDS)
    double* out = part + (int64_t)blockIdx.x * (d + 2);
    for (int s = 0; s < nslab; ++s) {
        const int k0 = s * HY_SLAB, kc = min(HY_SLAB, d - k0);
        if (nslab > 1) {
            __syncthreads();
            stage(k0, kc);
            __syncthreads();
        }
        for (int k = 0; k < kc; ++k) {
            double b4[4], sum = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) b4[j] = xj[k * HY_PITCH + colv[j]];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double a = xi[k * HY_PITCH + acc_row(i, r)];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double df = a - b4[j];
                        sum = fma(acc[i][j][r], df * df, sum);
                    }
                }
            sum = hy_wave_sum(sum);
            if (lane == 0) red[w * (HY_SLAB + 2) + k] = sum;
        }
        __syncthreads();
        if (t < kc) out[2 + k0 + t] = (red[t] + red[(HY_SLAB + 2) + t]) + (red[2 * (HY_SLAB + 2) + t] + red[3 * (HY_SLAB + 2) + t]);
        if (s == 0 && t >= HY_SLAB && t < HY_SLAB + 2)
            out[t - HY_SLAB] = (red[t] + red[(HY_SLAB + 2) + t]) + (red[2 * (HY_SLAB + 2) + t] + red[3 * (HY_SLAB + 2) + t]);
    }
}

// res[1 + c]: component c of [sn2, rho, ell_1..d, bias] from the tiles' slots, added in slot order per thread, then over the
// workgroup in a fixed order; workgroup d + 2 sums alpha.  grid (d + 3)
__global__ __launch_bounds__(256) void k_loglik_grad_reduce(const double* __restrict__ part, int64_t ntiles, int d,
                                                            const double* __restrict__ alpha, int64_t N, double rho,
                                                            const double* __restrict__ invell, double* __restrict__ res) {
    __shared__ double sh[4];
    const int c = blockIdx.x, t = threadIdx.x;
    double v = 0.0;
    if (c < d + 2) {
        for (int64_t i = t; i < ntiles; i += 256) v += part[i * (d + 2) + c];
    } else {
        for (int64_t i = t; i < N; i += 256) v += alpha[i];
    }
    v = hy_wave_sum(v);
    if ((t & 63) == 0) sh[t >> 6] = v;
    __syncthreads();
    if (t != 0) return;
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    if (c == 0) res[1] = 0.5 * v;
    else if (c == 1) res[2] = 0.5 * v / rho;
    else if (c < d + 2) res[1 + c] = -invell[c - 2] * v;
    else res[3 + d] = v;
}

int loglik_grad_host(gpx_handle* h, double* loglik, double* grad) {
    if (!h->fitted) { h->err = "loglik_grad: model is not fitted"; return GPX_ESTATE; }
    if (!grad) { h->err = "loglik_grad: NULL gradient output"; return GPX_EARG; }
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GPX_EHIP; }
    if (int rc0 = ensure_inverse(h)) return rc0;
    const int d = (int)h->d, nP = (int)(h->Np / NB);
    const int64_t ntiles = (int64_t)nP * (nP + 1) / 2;
    const int64_t capP = h->cap_np / NB;             // sized for the handle's capacity
    if (int rc = ensure(h, h->dhyper, h->cap_hyper, hyper_ws(WsCarver(nullptr), capP * (capP + 1) / 2, h->cap_d).bytes / 8, "loglik_grad")) return rc;
    const HyperWs hw = hyper_ws(WsCarver(h->dhyper), ntiles, d);
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(k_loglik_grad_tiles, dim3((unsigned)ntiles), dim3(GEMM_THREADS), 0, s, h->dT, h->Np, nP, h->N, h->dXs, d,
                       h->dalpha, h->kernel_id, h->rho, hw.part);
    hipLaunchKernelGGL(k_loglik_grad_reduce, dim3((unsigned)(d + 3)), dim3(256), 0, s, hw.part, ntiles, d, h->dalpha, h->N, h->rho,
                       h->dinvell, hw.res);
    launch_loglik(h, hw.res);
    std::vector<double> host((size_t)d + 4);
    if (hipMemcpyAsync(host.data(), hw.res, host.size() * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
        h->err = "loglik_grad: kernel or D2H copy failed";
        return GPX_EHIP;
    }
    if (loglik) *loglik = host[0];
    for (int c = 0; c < d + 3; ++c) grad[c] = host[1 + c];
    return GPX_OK;
}

}  // namespace gpx
