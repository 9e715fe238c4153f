// kernels_path.hip -- pathwise Thompson sampling on gfx950: draws that honour the data (Matheron's rule; Wilson et al. 2020,
// "Efficiently sampling functions from Gaussian process posteriors").
//
// A draw is the random-feature PRIOR sample of kernels_rff.hip corrected exactly with the factorisation the handle holds:
//     f_s(x) = bias + sum_j theta_sj cos(W_sj . x + b_sj)  +  sum_{i < nv} v_si k(x, X_i)
//     v_s = (K + sn2 I)^-1 r_s,   r_s = (y - bias) - Phi_s(X) theta_s - sqrt(sn2) eps_s
// gpx_path_weights (api.hip): the prior at the observations by the Thompson sweep kernel over the handle's own inputs, r by
// k_path_resid as k-major panels of 128 draws, v = U (T r) by the joint posterior's and the knowledge gradient's panel products
// (k_cov_trmm, k_kg_solve), k_path_gather back to (S, N).
// gpx_path_sweep: the Thompson sweep kernel leaves bias + the feature sum in the value buffer; k_path_update adds the second sum --
// an (S x nv) . (nv x M) product whose right operand, the cross-Gram k(X, Xc), is formed tile by tile on the VALU (xgram_core.h and
// kern_eval: k_cross_gram's own expressions) and never leaves the compute unit.
#include "gemm_core.h"
#include "gpx_internal.h"
#include "gpx_math.h"
#include "xgram_core.h"

namespace gpx {

// ------------------------------------------------------------------------------------------------
// The weight panel in fragment order (ws_layout.h: path_frag_words).  Group g holds the draws 64 g .. 64 g + 16 njb - 1; its part
// is [tile][k-step][block of 16 draws][lane]: lane l of that fragment is v[draw = 64 g + 16 jb + (l & 15)][row = 64 tile + 4 kk + (l >> 4)],
// the A operand of v_mfma_f64_16x16x4 (gemm_core.h).  Rows >= nv and draws >= S are zeros: the padding is the mask.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_path_prep(const double* __restrict__ v, int64_t S, int64_t nv, int64_t g, int njb,
                                                   int64_t words, double* __restrict__ frag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= words) return;
    const int lane = (int)(e & 63);
    const int64_t q = e >> 6;
    const int jb = (int)(q % njb);
    const int64_t step = q / njb;                      // 16 tile + kk
    const int64_t draw = g * PATH_GROUP + jb * 16 + (lane & 15), row = step * 4 + (lane >> 4);
    frag[e] = (draw < S && row < nv) ? v[draw * nv + row] : 0.0;
}

// ------------------------------------------------------------------------------------------------
// vals[draw][m] += sum_{i < nv} v[draw][i] k(X_i, x_m) for one group of 16 NJB draws and the workgroup's 128 candidates.
//   * the VALU forms the 64 x 128 tile of covariances (8 x 4 entries per thread, as k_cross_gram) and writes it to LDS in the order
//     the B operand is read: [k-step kk][block of 16 candidates cb][lane], the 32-byte pieces of a 512-byte fragment XORed with cb so
//     that the eight candidate blocks a store instruction touches fall on different banks (a fragment read still covers its 512 bytes
//     once: conflict-free);
//   * wave w owns the candidates 32 w .. 32 w + 31 (two blocks) and all NJB draw blocks: 2 NJB accumulators that stay in registers
//     across the whole row loop; the A fragments come straight from the panel in global memory (512 contiguous bytes per wave and
//     fragment, the same for all four waves);
//   * TWO images of the tile: tile rt + 1 is formed while the matrix instructions of tile rt are in flight, one barrier per tile;
//   * one workgroup finishes its candidates alone, rows ascending, no atomics: a value depends on its draw's weights and its
//     candidate's coordinates only -- not on S, the draw's place in its group, M or the launch.
// LDS: 2 x 64 KiB images + xo (8 KiB) + xc (16 KiB) = 152 KiB: one workgroup per compute unit.
// ------------------------------------------------------------------------------------------------
constexpr int PATH_IMG = XK * XN;                                          // doubles of one image
constexpr size_t PATH_LDS_BYTES = (size_t)(2 * PATH_IMG + XDC * XK + XDC * XN) * sizeof(double);

template <int KID, int NJB>
__global__ __launch_bounds__(256, 1) void k_path_update(const double* __restrict__ Xs, int ntile, int d,
                                                        const double* __restrict__ Xc, int64_t M,
                                                        const double* __restrict__ invell, double rho,
                                                        const double* __restrict__ frag, int64_t s0, int ns,
                                                        double* __restrict__ vals) {
    extern __shared__ __attribute__((aligned(32))) double lds[];   // img[2][PATH_IMG] | xo[XDC][XK] | xc[XDC][XN]
    double (*xo)[XK] = reinterpret_cast<double (*)[XK]>(lds + 2 * PATH_IMG);
    double (*xc)[XN] = reinterpret_cast<double (*)[XN]>(lds + 2 * PATH_IMG + XDC * XK);
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const int lane = t & 63, w = t >> 6, fr = lane & 15, fk = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * XN;
    const bool onepass = (d <= XDC);
    if (onepass) xgram_stage_cand(xc, Xc, m0 + (t & (XN - 1)), M, d, invell, 0, d);
    // tile rt of k(X, Xc) -> image `img` (every entry finite: padding rows of Xs and candidates >= M are zero vectors)
    auto form = [&](int rt, double* img) {
        double r2[8][4];
        xgram_tile_r2(xo, xc, Xs, (int64_t)rt * XK, d, Xc, m0, M, invell, onepass, r2);
        const int cb = tx >> 2;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int row = ty * 8 + a;               // kk = row >> 2, the lane's k index row & 3
            d4 o;
#pragma unroll
            for (int b = 0; b < 4; ++b) o[b] = kern_eval(KID, r2[a][b], rho);
            const int piece = (((row & 3) << 2) | (tx & 3)) ^ cb;
            *reinterpret_cast<d4*>(img + (((row >> 2) * 8 + cb) << 6) + (piece << 2)) = o;
        }
    };
    d4 acc[NJB][2];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) acc[jb][0] = acc[jb][1] = (d4){0.0, 0.0, 0.0, 0.0};
    // the lane's element of the B fragment (kk, cb = 2 w + c): piece fk 4 + (fr >> 2), word fr & 3
    int boff[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int cb = 2 * w + c;
        boff[c] = (cb << 6) + ((((fk << 2) | (fr >> 2)) ^ cb) << 2) + (fr & 3);
    }
    form(0, lds);
    __syncthreads();
    for (int rt = 0; rt < ntile; ++rt) {
        const double* img = lds + (rt & 1) * PATH_IMG;
        const double* af = frag + (int64_t)rt * (XK / 4) * NJB * 64 + lane;
        double a[XK / 4][NJB];
#pragma unroll
        for (int kk = 0; kk < XK / 4; ++kk)
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) a[kk][jb] = af[(kk * NJB + jb) * 64];
        if (rt + 1 < ntile) form(rt + 1, lds + ((rt + 1) & 1) * PATH_IMG);
#pragma unroll
        for (int kk = 0; kk < XK / 4; ++kk) {
            const double b0 = img[(kk << 9) + boff[0]], b1 = img[(kk << 9) + boff[1]];
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) {
                acc[jb][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk][jb], b0, acc[jb][0], 0, 0, 0);
                acc[jb][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk][jb], b1, acc[jb][1], 0, 0, 0);
            }
        }
        __syncthreads();      // image rt & 1 has been read, image (rt + 1) & 1 is complete
    }
    // D[draw = fk + 4 r][candidate = fr]: (bias + feature sum) + update, in this order
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t gm = m0 + (2 * w + c) * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = jb * 16 + fk + 4 * r;
                if (q < ns && gm < M) {
                    double* o = vals + (s0 + q) * M + gm;
                    *o = *o + acc[jb][c][r];
                }
            }
        }
}

// v: the device copy of the caller's weights (S, nv); frag: the panel (path_sweep_ws).  Xs: the handle's scaled inputs, whose rows
// [0, 64 ceil(nv / 64)) exist (nv <= N <= Np, a multiple of 128).  vals (S, M) holds the feature part on entry.
void launch_path_update(hipStream_t s, const double* Xs, int d, const double* v, int64_t nv, int64_t S, double* frag,
                        const double* Xc, int64_t M, const double* invell, int kernel_id, double rho, double* vals) {
    const int ntile = (int)path_tiles(nv);
    const dim3 grid((unsigned)((M + XN - 1) / XN));
    const int64_t G = (S + PATH_GROUP - 1) / PATH_GROUP;
    for (int64_t g = 0; g < G; ++g) {
        const int njb = path_group_blocks(S, g);
        const int64_t words = (int64_t)ntile * (XK / 4) * njb * 64;
        double* fg = frag + path_group_offset(nv, g);
        hipLaunchKernelGGL(k_path_prep, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, v, S, nv, g, njb, words, fg);
        const int64_t s0 = g * PATH_GROUP;
        const int ns = (int)std::min<int64_t>(PATH_GROUP, S - s0);
#define GPX_PU(KID, NJB)                                                                                                                   \
        do {                                                                                                                               \
            hipFuncSetAttribute((const void*)k_path_update<KID, NJB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PATH_LDS_BYTES);    \
            hipLaunchKernelGGL((k_path_update<KID, NJB>), grid, dim3(256), PATH_LDS_BYTES, s, Xs, ntile, d, Xc, M, invell, rho, fg, s0, ns, vals); \
        } while (0)
#define GPX_PUK(KID)                                                                                                                       \
        switch (njb) {                                                                                                                     \
            case 1: GPX_PU(KID, 1); break;                                                                                                 \
            case 2: GPX_PU(KID, 2); break;                                                                                                 \
            case 3: GPX_PU(KID, 3); break;                                                                                                 \
            default: GPX_PU(KID, 4); break;                                                                                                \
        }
        switch (kernel_id) {
            case GPX_KERN_SE_ARD: GPX_PUK(GPX_KERN_SE_ARD); break;
            case GPX_KERN_MATERN52: GPX_PUK(GPX_KERN_MATERN52); break;
            case GPX_KERN_MATERN32: GPX_PUK(GPX_KERN_MATERN32); break;
            default: GPX_PUK(GPX_KERN_MATERN12); break;
        }
#undef GPX_PUK
#undef GPX_PU
    }
}

// ------------------------------------------------------------------------------------------------
// The right-hand sides of gpx_path_weights as k-major panels of 128 draws, R[p][i][c] for draw s = 128 p + c:
//     r_si = ((y_i - bias) - prior_si) - sqrt(sn2) eps_si      (eps null: the last term is left out); 0 for i >= N or s >= S
// and the way back from the panels of U T r to v (S, N).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void k_path_resid(const double* __restrict__ y, double bias, const double* __restrict__ prior,
                                                   const double* __restrict__ eps, double sn, int64_t S, int64_t N, int64_t Np,
                                                   double* __restrict__ R) {
    const int64_t i = blockIdx.x, p = blockIdx.y, s = p * TB + threadIdx.x;
    double r = 0.0;
    if (i < N && s < S) {
        r = (y[i] - bias) - prior[s * N + i];
        if (eps) r = r - sn * eps[s * N + i];
    }
    R[(p * Np + i) * TB + threadIdx.x] = r;
}

__global__ __launch_bounds__(256) void k_path_gather(const double* __restrict__ Wp, int64_t S, int64_t N, int64_t Np,
                                                     double* __restrict__ v) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= S * N) return;
    const int64_t s = e / N, i = e - s * N;
    v[e] = Wp[((s / TB) * Np + i) * TB + (s % TB)];
}

void launch_path_resid(hipStream_t s, const double* y, double bias, const double* prior, const double* eps, double sn, int64_t S,
                       int64_t N, int64_t Np, int64_t Sp, double* R) {
    hipLaunchKernelGGL(k_path_resid, dim3((unsigned)Np, (unsigned)(Sp / TB)), dim3(TB), 0, s, y, bias, prior, eps, sn, S, N, Np, R);
}

void launch_path_gather(hipStream_t s, const double* Wp, int64_t S, int64_t N, int64_t Np, double* v) {
    hipLaunchKernelGGL(k_path_gather, dim3((unsigned)((S * N + 255) / 256)), dim3(256), 0, s, Wp, S, N, Np, v);
}

}  // namespace gpx
