// kernels_cov.hip -- the JOINT posterior at a point set on gfx950: full covariance and exact draws.
//
// What a duck-typed reggie model offers as `model.sample(X, ...)` / a `predict` with the full covariance (the reference's
// demos draw sample paths of the posterior with it); every other entry point of the engine returns marginals.  For M <= 4096
// points Z (api.hip: joint_core):
//   1. k_cross_gram   Ks[nt][k][c] = k(x_k, z_{128 nt + c}): the sweep's own kernel, so K* has the sweep's bits
//   2. k_cov_trmm     V = T Ks on fp64 MFMA, tile (mt, nt), K-extent (mt + 1) 128 as in the sweep -- but the epilogue STORES the
//                     tile, panel-major V[nt][Np][128]: every 128-column panel of V is a k-major operand of step 4
//   3. k_cov_mu_part / k_cov_mu   mu = bias + V^T a: per 128-row block partial sums, added in block order (fixed order, no atomics)
//   4. k_cov_syrk     Sigma = k(Z, Z) - V^T V: one workgroup per lower 128-tile (I, J), J <= I, contraction over all Np rows of V
//                     in ascending order; k(Z, Z) comes from k_cross_gram on the scaled points (same layout as Ks); the epilogue only
//                     stores: the tile and its mirror image (inside diagonal tiles the entries on and below the diagonal and their
//                     copies), so the matrix is symmetric bit for bit
//   5. k_cov_form     B = Sigma + c I into an (Mp, Mp) buffer with identity padding (what launch_cholesky_small factors: B = R^T R)
//   6. k_cov_draw     out[s][j] = mu[j] + sum_{i <= j} z[s][i] R[i][j], i ascending whatever S is
#include "gemm_core.h"
#include "gpx_internal.h"

namespace gpx {

// Tile (mt, nt) of V = T Ks, heavy tiles (large mt) first.  U, Ks as in k_sweep_trmm_l (both k-major; the all-zero quarter-rows
// of T's diagonal block are skipped).  Padding rows of T are identity rows and padding rows / columns of Ks are zeros: the
// padding of V is exact zeros.
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_cov_trmm(const double* __restrict__ U, int64_t Np,
                                                              const double* __restrict__ Ks, int NT, double* __restrict__ V) {
    __shared__ __attribute__((aligned(16))) double smem[gemm_l_lds_f64<32>()];
    const int nP = (int)(Np / TB);
    const int mt = nP - 1 - (int)blockIdx.x / NT, nt = (int)blockIdx.x % NT;
    const int64_t m0 = (int64_t)mt * TB;
    d4 acc[4][4];
    acc_zero(acc);
    gemm_tile_128_l<32, 1, 2, true, true>(acc, U + m0, Np, Ks + (int64_t)nt * Np * TB, TB, 0, (mt + 1) * TB, smem);
    double* Vt = V + ((int64_t)nt * Np + m0) * TB;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* row = Vt + acc_row_ilv(i, r) * TB;
#pragma unroll
            for (int j = 0; j < 4; ++j) row[acc_col(j)] = acc[i][j][r];
        }
}

void launch_cov_trmm(hipStream_t s, const double* U, int64_t Np, const double* Ks, int64_t cols, double* V) {
    const int NT = (int)(cols / TB);
    hipLaunchKernelGGL(k_cov_trmm, dim3((unsigned)(Np / TB * NT)), dim3(GEMM_THREADS), 0, s, U, Np, Ks, NT, V);
}

// mu = bias + V^T a in two steps: Pp[mt][j] = sum over the rows of block mt (ascending), then the blocks in order
__global__ __launch_bounds__(TB) void k_cov_mu_part(const double* __restrict__ V, int64_t Np, const double* __restrict__ a,
                                                    double* __restrict__ Pp, int64_t ldp) {
    const int nt = blockIdx.x, mt = blockIdx.y, c = threadIdx.x;
    const double* v = V + ((int64_t)nt * Np + (int64_t)mt * TB) * TB + c;
    const double* av = a + (int64_t)mt * TB;
    double p = 0.0;
    for (int k = 0; k < TB; ++k) p = fma(v[(int64_t)k * TB], av[k], p);
    Pp[(int64_t)mt * ldp + (int64_t)nt * TB + c] = p;
}

__global__ __launch_bounds__(256) void k_cov_mu(const double* __restrict__ Pp, int nP, int64_t ldp, int64_t Mp, double bias,
                                                double* __restrict__ mu) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Mp) return;
    double p = 0.0;
    for (int mt = 0; mt < nP; ++mt) p += Pp[(int64_t)mt * ldp + j];
    mu[j] = bias + p;
}

void launch_cov_mu(hipStream_t s, const double* V, int64_t Np, int64_t cols, const double* a, double bias, double* Pp,
                   double* mu) {
    const int nP = (int)(Np / TB);
    hipLaunchKernelGGL(k_cov_mu_part, dim3((unsigned)(cols / TB), (unsigned)nP), dim3(TB), 0, s, V, Np, a, Pp, cols);
    hipLaunchKernelGGL(k_cov_mu, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, Pp, nP, cols, cols, bias, mu);
}

// Tile (I, J) = (blockIdx.y, blockIdx.x), J <= I, of C = Kss - V^T V.  V's panels I and J are the k-major operands (pitch 128),
// Kss[J][row][col] = k(z_row, z_{128 J + col}) (pitch Mp rows per panel); C (Mp, Mp) row-major.  RAW: no clamp on the diagonal.
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_cov_syrk(const double* __restrict__ V, int64_t Np,
                                                              const double* __restrict__ Kss, int64_t Mp, double* __restrict__ C) {
    __shared__ __attribute__((aligned(16))) double smem[gemm_l_lds_f64<32>()];
    const int I = blockIdx.y, J = blockIdx.x;
    if (J > I) return;
    d4 acc[4][4];
    acc_zero(acc);
    gemm_tile_128_l<32, 1, 2>(acc, V + (int64_t)I * Np * TB, TB, V + (int64_t)J * Np * TB, TB, 0, (int)Np, smem);
    const double* Kt = Kss + ((int64_t)J * Mp + (int64_t)I * TB) * TB;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = acc_row(i, r);
            const int64_t gi = (int64_t)I * TB + row;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = acc_col(j);
                const int64_t gj = (int64_t)J * TB + col;
                if (I != J || col <= row) {
                    const double v = Kt[row * TB + col] - acc[i][j][r];
                    C[gi * Mp + gj] = v;
                    C[gj * Mp + gi] = v;
                }
            }
        }
}

void launch_cov_syrk(hipStream_t s, const double* V, int64_t Np, const double* Kss, int64_t Mp, double* C) {
    const unsigned nt = (unsigned)(Mp / TB);
    hipLaunchKernelGGL(k_cov_syrk, dim3(nt, nt), dim3(GEMM_THREADS), 0, s, V, Np, Kss, Mp, C);
}

// B = C + add I on the leading M x M part, identity padding (the layout launch_cholesky_small factors; it consumes B)
__global__ __launch_bounds__(256) void k_cov_form(const double* __restrict__ C, int64_t M, int64_t Mp, double add,
                                                  double* __restrict__ B) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Mp * Mp) return;
    const int64_t i = idx / Mp, j = idx - i * Mp;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < M && j < M) v = (i == j) ? C[idx] + add : C[idx];
    B[idx] = v;
}

void launch_cov_form(hipStream_t s, const double* C, int64_t M, int64_t Mp, double add, double* B) {
    hipLaunchKernelGGL(k_cov_form, dim3((unsigned)((Mp * Mp + 255) / 256)), dim3(256), 0, s, C, M, Mp, add, B);
}

// out[s][j] = mu[j] + sum_{i <= j} z[s][i] R[i][j].  Workgroup (jb, sg): 128 columns x DRAW_S draws; a thread owns one column and
// walks the rows i = 0 .. j in ascending order (a draw's bits do not depend on S or on its place in the batch), the wave reads
// each row of R as consecutive doubles, and the 128-row slices of the group's z rows pass through LDS once per column block.
// Nothing is written when the factorisation failed (*flag != 0).
constexpr int DRAW_S = 8;

__global__ __launch_bounds__(TB) void k_cov_draw(const double* __restrict__ R, int64_t Mp, int64_t M, const double* __restrict__ z,
                                                 int64_t S, const double* __restrict__ mu, const int* __restrict__ flag,
                                                 double* __restrict__ out) {
    __shared__ double zs[DRAW_S][TB];
    if (*flag != 0) return;
    const int jb = blockIdx.x, c = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.y * DRAW_S, j = (int64_t)jb * TB + c;
    double acc[DRAW_S];
#pragma unroll
    for (int q = 0; q < DRAW_S; ++q) acc[q] = 0.0;
    for (int ib = 0; ib <= jb; ++ib) {
        const int64_t i0 = (int64_t)ib * TB;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < DRAW_S; ++q) zs[q][c] = (s0 + q < S && i0 + c < M) ? z[(s0 + q) * M + i0 + c] : 0.0;
        __syncthreads();
        const int kend = (ib == jb) ? c + 1 : TB;
        const double* Rc = R + i0 * Mp + j;
        for (int k = 0; k < kend; ++k) {
            const double r = Rc[(int64_t)k * Mp];
#pragma unroll
            for (int q = 0; q < DRAW_S; ++q) acc[q] = fma(zs[q][k], r, acc[q]);
        }
    }
    if (j < M) {
        const double m = mu[j];
#pragma unroll
        for (int q = 0; q < DRAW_S; ++q)
            if (s0 + q < S) out[(s0 + q) * M + j] = m + acc[q];
    }
}

void launch_cov_draw(hipStream_t s, const double* R, int64_t Mp, int64_t M, const double* z, int64_t S, const double* mu,
                     const int* flag, double* out) {
    const int64_t per = (int64_t)65535 * DRAW_S;          // draws per launch (grid.y)
    for (int64_t q0 = 0; q0 < S; q0 += per) {
        const int64_t n = S - q0 < per ? S - q0 : per;
        hipLaunchKernelGGL(k_cov_draw, dim3((unsigned)(Mp / TB), (unsigned)((n + DRAW_S - 1) / DRAW_S)), dim3(TB), 0, s, R, Mp, M,
                           z + q0 * M, n, mu, flag, out + q0 * M);
    }
}

}  // namespace gpx
