// kernels_kg.hip -- the knowledge gradient over a support set (GPX_ACQ_KG, gpx_kg_grad; the mathematics: kg_math.h).
// A translation unit of its own, as kernels_mes.hip: kernels_sweep.hip, acq_value and k_acq stay textually what they were.
//
// A candidate z is scored by the expected rise of the maximum posterior mean over {z} + A after one noisy observation at z.  Lines:
//   line 0      a_0 = mu(z),    b_0 = s2(z) / D,            D = sqrt(s2(z) + sn2)
//   line j      a_j = mu(a_j),  b_j = Sigma(a_j, z) / D,    Sigma(a_j, z) = k(z, a_j) - Ks_z . B_j,   B = (K + sn2 I)^-1 k(X, A)
// Once per support set (api.hip: kg_prepare): Ks_A by the sweep's cross-Gram kernel, V_A = T Ks_A (k_cov_trmm), a_j = bias + V_A^T a
// (launch_cov_mu), B = U V_A (k_kg_solve) as ONE k-major panel [Np][128] whose rows N .. Np - 1 and columns m .. 127 are exact zeros.
// Per chunk of a sweep:
//   k_kg_cross   C[j][c] = sum_n B[n][j] Ks[panel(c)][n][c]: one workgroup per candidate panel on gemm_tile_128_l, all Np rows ascending
//   k_acq_kg     k_acq's moments, then k(z, a_j), the lines and kg_math.h
// For gpx_kg_grad's points (panels of 128): Ks_z, V_z = T Ks_z, W_z = U V_z by the same kernels, then
//   k_kg_point_sums   per (point, coordinate): sum_n e_n E[n][.] over E = [B | alpha | W_z] with e_n = k(z, x_n) or d/dz_t k(z, x_n)
//   k_kg_point_final  lines, value, per-line weights (kg_weights) and the gradient
#include "gemm_core.h"
#include "gpx_internal.h"
#include "gpx_math.h"
#include "acq_core.h"
#include "kg_math.h"

namespace gpx {

constexpr int KG_PANEL = KG_MAX_LINES;      // 128: the support panel's columns
constexpr int KG_CB = 64;                   // candidates per workgroup of k_acq_kg / k_kg_point_final (x KG_WAYS threads each)
constexpr int KG_EC = 132;                  // columns of a point's sums: [0, 128) B, 128 alpha, 129 W_z, 130 sum V_z^2, 131 unused

// squared scaled distance between a scaled support point and a raw point: the cross-Gram's statements (the product z invell rounds on
// its own, the first square is a product, the rest FMAs)
__device__ __forceinline__ double kg_r2(const double* __restrict__ as, const double* __restrict__ z, const double* __restrict__ invell,
                                        int d) {
    double r2 = 0.0;
    for (int k = 0; k < d; ++k) {
        double zs;
        {
#pragma clang fp contract(off)
            zs = z[k] * invell[k];
        }
        const double df = as[k] - zs;
        r2 = (k == 0) ? df * df : fma(df, df, r2);
    }
    return r2;
}

// W[n][j] = sum_{k >= n} U[n][k] V[k][j], k ascending: row n of W = U V for one panel V [Np][128] (U = R^-1 upper, row-major).
// One workgroup per row, one thread per column.  Rows n >= N and columns j >= m are written as exact zeros.
__global__ __launch_bounds__(KG_PANEL) void k_kg_solve(const double* __restrict__ U, int64_t Np, int64_t N, int m,
                                                       const double* __restrict__ V, double* __restrict__ W) {
    const int64_t n = blockIdx.x;
    const int j = threadIdx.x;
    double acc = 0.0;
    if (n < N && j < m) {
        const double* u = U + n * Np;
        for (int64_t k = n; k < N; ++k) acc = fma(u[k], V[k * KG_PANEL + j], acc);
    }
    W[n * KG_PANEL + j] = acc;
}

void launch_kg_solve(hipStream_t s, const double* U, int64_t Np, int64_t N, int m, const double* V, double* W) {
    hipLaunchKernelGGL(k_kg_solve, dim3((unsigned)Np), dim3(KG_PANEL), 0, s, U, Np, N, m, V, W);
}

// C[j][128 nt + c] = sum_n B[n][j] Ks[nt][n][c] for candidate panel nt = blockIdx.x: B and the panel are both k-major operands of
// pitch 128, K-extent Np in ascending 32-row steps (the padding rows of both are zeros).  C has the pitch ldc (the chunk's columns).
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_kg_cross(const double* __restrict__ B, int64_t Np, const double* __restrict__ Ks,
                                                              int64_t ldk, double* __restrict__ C, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) double smem[gemm_l_lds_f64<32>()];
    const int nt = blockIdx.x;
    d4 acc[4][4];
    acc_zero(acc);
    gemm_tile_128_l<32, 1, 2>(acc, B, TB, Ks + (int64_t)nt * ldk * TB, TB, 0, (int)Np, smem);
    double* Ct = C + (int64_t)nt * TB;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* row = Ct + (int64_t)acc_row(i, r) * ldc;
#pragma unroll
            for (int j = 0; j < 4; ++j) row[acc_col(j)] = acc[i][j][r];
        }
}

void launch_kg_cross(hipStream_t s, const double* B, int64_t Np, const double* Ks, int64_t ldk, int64_t cols, double* C, int64_t ldc) {
    hipLaunchKernelGGL(k_kg_cross, dim3((unsigned)(cols / TB)), dim3(GEMM_THREADS), 0, s, B, Np, Ks, ldk, C, ldc);
}

// the lines of one candidate: line 0 in registers, the support lines' intercepts in global memory (the line index is uniform over a
// wave: scalar loads) and their slopes in LDS, [line - 1][candidate of the workgroup]
struct KgLdsLines {
    double a0, b0;
    const double* al;
    const double* be;
    __device__ __forceinline__ double a(int i) const { return i == 0 ? a0 : al[i - 1]; }
    __device__ __forceinline__ double b(int i) const { return i == 0 ? b0 : be[(i - 1) * KG_CB]; }
};

// k_acq (kernels_sweep.hip) with another last part and another workgroup shape: the sums and moments are cand_moments' (acq_core.h), so
// they -- and the sums a sweep cache is seeded with -- are the bits every other acquisition returns.
// Workgroup: KG_CB candidates x KG_WAYS waves; wave t forms the slopes of the support points t, t + 4, .. and the partial sum of the
// lines t, t + 4, .. (kg_partial); wave 0 combines.  Every wave forms the moments (a few loads), wave 0 stores them.  A candidate's
// value depends on its coordinates and the support set alone: nothing here reads the chunk, the panel or the lane but to find the
// candidate's own column.  X: the candidate array the chunk's columns index with m0 + n (raw coordinates).
__global__ __launch_bounds__(KG_CB* KG_WAYS) void k_acq_kg(const double* __restrict__ Qp, const double* __restrict__ Pp, int64_t ldp,
                                                           int nrb, int64_t m0, int64_t cols_valid, double rho, double bias,
                                                           double sn2, int kid, int d, const double* __restrict__ X,
                                                           const double* __restrict__ invell, const double* __restrict__ As, int m,
                                                           const double* __restrict__ al, const double* __restrict__ C, int64_t ldc,
                                                           double* __restrict__ acq_out, double* __restrict__ mu_out,
                                                           double* __restrict__ s2_out, double* __restrict__ qsum,
                                                           double* __restrict__ psum) {
    __shared__ double be[KG_MAX_M * KG_CB];
    const int c = threadIdx.x & (KG_CB - 1), t = threadIdx.x / KG_CB;
    const int64_t n = (int64_t)blockIdx.x * KG_CB + c;
    const bool live = n < cols_valid;
    KgLdsLines ln = {0.0, 0.0, al, be + c};
    if (live) {
        const CandMoments cm = cand_moments(Qp, Pp, ldp, nrb, n, rho, bias);
        const double mu = cm.mu, s2 = cm.s2;
        if (qsum && t == 0) {
            qsum[m0 + n] = cm.q;
            psum[m0 + n] = cm.p;
        }
        if (t == 0) {
            if (mu_out) mu_out[m0 + n] = mu;
            if (s2_out) s2_out[m0 + n] = s2;
        }
        const double D = sqrt(s2 + sn2);
        ln.a0 = mu;
        ln.b0 = s2 / D;
        const double* z = X + (m0 + n) * d;
        for (int j = t; j < m; j += KG_WAYS) {
            const double kz = kern_eval(kid, kg_r2(As + (int64_t)j * d, z, invell, d), rho);
            be[j * KG_CB + c] = (kz - C[(int64_t)j * ldc + n]) / D;
        }
    }
    __syncthreads();
    const double part = live ? kg_partial(t, m + 1, ln, ln.b0) : 0.0;
    __syncthreads();                       // every slope has been read: the partial sums take their place
    be[t * KG_CB + c] = part;
    __syncthreads();
    if (t == 0 && live) {
        const double p4[KG_WAYS] = {be[c], be[KG_CB + c], be[2 * KG_CB + c], be[3 * KG_CB + c]};
        acq_out[m0 + n] = kg_combine(p4);
    }
}

void launch_acq_kg(hipStream_t s, const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t m0, int64_t cols_valid,
                   double rho, double bias, double sn2, int kid, int d, const double* X, const double* invell, const double* As, int m,
                   const double* al, const double* C, int64_t ldc, double* acq_out, double* mu_out, double* s2_out, double* qsum,
                   double* psum) {
    const unsigned g = (unsigned)((cols_valid + KG_CB - 1) / KG_CB);
    hipLaunchKernelGGL(k_acq_kg, dim3(g), dim3(KG_CB * KG_WAYS), 0, s, Qp, Pp, ldp, nrb, m0, cols_valid, rho, bias, sn2, kid, d, X,
                       invell, As, m, al, C, ldc, acq_out, mu_out, s2_out, qsum, psum);
}

// ---- gpx_kg_grad ---------------------------------------------------------------------------------------------------------------
// Sums of point p = blockIdx.x of a panel over the observed rows, n ascending, for coordinate t = blockIdx.y (t = d: the values):
//     S[p][t][col] = sum_n e_n E[n][col],   e_n = k(z, x_n)  (t = d)   or   d/dz_t k(z, x_n) = g_n 2 invell_t (zs_t - xs_nt)  (t < d),
// E = [B (128) | alpha | W_z[.][p]]; for t = d column 130 holds sum_n V_z[n][p]^2 (the sweep's q).  128 rows at a time: thread i < 128
// forms e of row n0 + i into LDS, then thread col adds the 128 products in order.  A row of the result does not depend on M.
__global__ __launch_bounds__(192) void k_kg_point_sums(const double* __restrict__ Xs, int64_t N, int d, const double* __restrict__ Z,
                                                       const double* __restrict__ invell, int kid, double rho,
                                                       const double* __restrict__ B, const double* __restrict__ alpha,
                                                       const double* __restrict__ Wz, const double* __restrict__ Vz,
                                                       double* __restrict__ S) {
    __shared__ double e[KG_PANEL];
    const int p = blockIdx.x, t = blockIdx.y, col = threadIdx.x;
    const double* z = Z + (int64_t)p * d;
    double acc = 0.0;
    for (int64_t n0 = 0; n0 < N; n0 += KG_PANEL) {
        __syncthreads();
        if (col < KG_PANEL) {
            const int64_t n = n0 + col;
            double v = 0.0;
            if (n < N) {
                double kv, gv;
                kern_and_grad(kid, kg_r2(Xs + n * d, z, invell, d), rho, kv, gv);
                v = kv;
                if (t < d) v = gv * (2.0 * invell[t] * (z[t] * invell[t] - Xs[n * d + t]));
            }
            e[col] = v;
        }
        __syncthreads();
        const int nn = (int)((N - n0 < KG_PANEL) ? N - n0 : KG_PANEL);
        if (col < KG_PANEL) {
            for (int i = 0; i < nn; ++i) acc = fma(e[i], B[(n0 + i) * KG_PANEL + col], acc);
        } else if (col == KG_PANEL) {
            for (int i = 0; i < nn; ++i) acc = fma(e[i], alpha[n0 + i], acc);
        } else if (col == KG_PANEL + 1) {
            for (int i = 0; i < nn; ++i) acc = fma(e[i], Wz[(n0 + i) * KG_PANEL + p], acc);
        } else if (col == KG_PANEL + 2 && t == d) {
            for (int i = 0; i < nn; ++i) {
                const double v = Vz[(n0 + i) * KG_PANEL + p];
                acc = fma(v, v, acc);
            }
        }
    }
    if (col < KG_EC) S[((int64_t)p * (d + 1) + t) * KG_EC + col] = acc;
}

void launch_kg_point_sums(hipStream_t s, const double* Xs, int64_t N, int d, const double* Z, int np, const double* invell, int kid,
                          double rho, const double* B, const double* alpha, const double* Wz, const double* Vz, double* S) {
    hipLaunchKernelGGL(k_kg_point_sums, dim3((unsigned)np, (unsigned)(d + 1)), dim3(192), 0, s, Xs, N, d, Z, invell, kid, rho, B,
                       alpha, Wz, Vz, S);
}

// the lines of one point in global scratch, [line][point of the panel]
struct KgGlobalLines {
    const double *al0, *al, *be;
    __device__ __forceinline__ double a(int i) const { return i == 0 ? *al0 : al[i - 1]; }
    __device__ __forceinline__ double b(int i) const { return be[i * KG_PANEL]; }
};

// Value and gradient of the np points of a panel from their sums.  Workgroup: KG_CB points x KG_WAYS ways, as k_acq_kg.  L: scratch
// [4][129][128]: slopes b_j, dk/dr2 of k(z, a_j), weights w_j; [3][0][.] the intercept of line 0, [3][1][.] P_0 - [0 = argmax a].
//     dKG/dz_t = (P_0 - [0 = argmax a]) dmu_t + w_0 db_0,t + sum_j w_j db_j,t,
//     db_0 = ds2 (1 / D - s2 / (2 D^3)),   db_j = dSigma_j / D - b_j ds2 / (2 D^2),   dSigma_j = d/dz k(z, a_j) - sum_n d/dz k(z, x_n) B[n][j].
__global__ __launch_bounds__(KG_CB* KG_WAYS) void k_kg_point_final(const double* __restrict__ S, int np, int d, const double* __restrict__ Z,
                                                                   const double* __restrict__ invell, const double* __restrict__ As,
                                                                   int m, const double* __restrict__ al, int kid, double rho,
                                                                   double bias, double sn2, double* __restrict__ L,
                                                                   double* __restrict__ f, double* __restrict__ g) {
    __shared__ double part[KG_WAYS * KG_CB];
    const int c = threadIdx.x & (KG_CB - 1), t = threadIdx.x / KG_CB;
    const int p = blockIdx.x * KG_CB + c;
    const bool live = p < np;
    const int64_t plane = (int64_t)(KG_MAX_LINES + 1) * KG_PANEL;
    double* be = L + p;
    double* gk = L + plane + p;
    double* wj = L + 2 * plane + p;
    double* misc = L + 3 * plane + p;
    const double* Sp = S + (int64_t)p * (d + 1) * KG_EC;
    const double* z = Z + (int64_t)p * d;
    double s2 = 1.0, D = 1.0;
    if (live) {
        const double* Sv = Sp + (int64_t)d * KG_EC;
        const double mu = bias + Sv[KG_PANEL];
        s2 = s2_floored(rho, Sv[KG_PANEL + 2]);
        D = sqrt(s2 + sn2);
        if (t == 0) {
            misc[0] = mu;
            be[0] = s2 / D;
        }
        for (int j = t; j < m; j += KG_WAYS) {
            double kv, gv;
            kern_and_grad(kid, kg_r2(As + (int64_t)j * d, z, invell, d), rho, kv, gv);
            be[(j + 1) * KG_PANEL] = (kv - Sv[j]) / D;
            gk[(j + 1) * KG_PANEL] = gv;
        }
    }
    __syncthreads();
    const KgGlobalLines ln = {misc, al, be};
    double ps = 0.0;
    if (live) {
        const double bref = ln.b(0);
        for (int j = t; j <= m; j += KG_WAYS) {
            ps += kg_term(j, m + 1, ln, bref);
            double P, w;
            kg_weights(j, m + 1, ln, P, w);
            wj[j * KG_PANEL] = w;
            if (j == 0) {
                bool top = true;
                for (int i = 1; i <= m; ++i) top = top && !(ln.a(i) > ln.a(0));
                misc[KG_PANEL] = P - (top ? 1.0 : 0.0);
            }
        }
    }
    part[t * KG_CB + c] = ps;
    __syncthreads();
    if (!live) return;
    if (t == 0) {
        const double p4[KG_WAYS] = {part[c], part[KG_CB + c], part[2 * KG_CB + c], part[3 * KG_CB + c]};
        f[p] = kg_combine(p4);
    }
    const double pm = misc[KG_PANEL], w0 = wj[0];
    const double db0 = 1.0 / D - s2 / (2.0 * D * D * D), h2 = 1.0 / (2.0 * D * D);
    for (int tc = t; tc < d; tc += KG_WAYS) {
        const double* St = Sp + (int64_t)tc * KG_EC;
        const double dmu = St[KG_PANEL], ds2 = -2.0 * St[KG_PANEL + 1];
        const double zs = z[tc] * invell[tc];
        double acc = pm * dmu + w0 * (ds2 * db0);
        for (int j = 1; j <= m; ++j) {
            const double dk = gk[j * KG_PANEL] * (2.0 * invell[tc] * (zs - As[(int64_t)(j - 1) * d + tc]));
            const double db = (dk - St[j - 1]) / D - be[j * KG_PANEL] * ds2 * h2;
            acc = fma(wj[j * KG_PANEL], db, acc);
        }
        g[(int64_t)p * d + tc] = acc;
    }
}

void launch_kg_point_final(hipStream_t s, const double* S, int np, int d, const double* Z, const double* invell, const double* As,
                           int m, const double* al, int kid, double rho, double bias, double sn2, double* L, double* f, double* g) {
    hipLaunchKernelGGL(k_kg_point_final, dim3((unsigned)((np + KG_CB - 1) / KG_CB)), dim3(KG_CB * KG_WAYS), 0, s, S, np, d, Z, invell,
                       As, m, al, kid, rho, bias, sn2, L, f, g);
}

}  // namespace gpx
