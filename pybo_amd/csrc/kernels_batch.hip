// kernels_batch.hip -- batch proposals (gpx_sweep_batch): nb greedy picks on the live sweep cache, each conditioned on the ones
// before it at their posterior mean (Kriging believer / GP-BUCB hallucination: the mean stays, the variance shrinks).
//
// With q' a scratch copy of the cache's q_n = |V(z_n)|^2, round j scores val_n = acq(bias + p_n, max(rho - q'_n, S2_FLOOR)), picks
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
// The order, the moments, batch_fold, a pick's scalars and the ensemble's fold and finish are acq_core.h's; block_argmax and the
// front of the pick kernels (merge_pick) acq_core_dev.h's.
//
// The ensemble forms (gpx_ensemble_sweep_batch: n members frozen for the batch, every member conditioned on the pick at ITS OWN
// posterior mean) keep the recurrence per member -- its own w, d, cross terms, 1/ell, V and q' -- and share the pick:
//   k_ens_batch_score  one pass with all members inside it: per member batch_fold (as k_batch_score), its value (EI / PI) or
//                      moments (UCB), summed in member order and divided once by k_ens_accum's and k_ens_finish's functions
//   k_ens_batch_pick   the pick, the raw x once, and per member s2, d, the cross terms, x / ell_m and sel_s2[m][j]
//   k_ens_same_grid    the members' caches hold the same candidates, bit for bit (one flag word, read at the call's only sync)
//
// The fantasised form (gpx_sweep_batch_fantasy: the pending outcomes integrated out by Monte Carlo instead of set to their mean)
// keeps the recurrence and replaces the value: k_fant_score, k_fant_pick, described where they stand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acq_core_dev.h"
#include "gpx_internal.h"
#include "gpx_math.h"

namespace gpx {

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
    double bv = NEG_INF;
    int64_t bi = IDX_NONE;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < M; n += stride) {
        double q;
        if (j < 0) {
            q = cq[n];
        } else {
            q = batch_fold(j, M, n, V, cross, scal[1], V[(int64_t)j * M + n], qp[n]);
        }
        qp[n] = q;
        const CandMoments c = moments_of_sums(q, cp[n], rho, bias);
        if (s2_out) s2_out[n] = c.s2;
        if (!taken[n]) {
            const double val = nan_last(acq_value(acq_id, c.mu, c.s2, p0));
            if (better(val, n, bv, bi)) { bv = val; bi = n; }
        }
    }
    block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        partv[blockIdx.x] = bv;
        parti[blockIdx.x] = bi;
    }
}

// scal: pick_scalars' four words
__global__ __launch_bounds__(256) void k_batch_pick(int j, int nblk, const double* __restrict__ partv,
                                                    const int64_t* __restrict__ parti, int64_t M, int d,
                                                    const double* __restrict__ Z, const double* __restrict__ invell,
                                                    const double* __restrict__ qp, const double* __restrict__ V, double rho,
                                                    double sn2, double* __restrict__ x, double* __restrict__ xs,
                                                    double* __restrict__ scal, double* __restrict__ cross,
                                                    double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                    double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    const int64_t row = merge_pick(j, nblk, partv, parti, M, sel_val, sel_idx, taken);
    const int t = threadIdx.x;
    if (t == 0) {
        const double s2 = s2_floored(rho, qp[row]);
        sel_s2[j] = s2;
        pick_scalars(s2, sn2, scal);
    }
    if (t < j) cross[t] = V[(int64_t)t * M + row];
    for (int k = t; k < d; k += 256) {
        const double xv = Z[row * d + k];
        x[k] = xv;
        xs[k] = xv * invell[k];
    }
}

// ---- fantasised picks (gpx_sweep_batch_fantasy) -----------------------------------------------------------------------------
// The believer's recurrence with the pending outcomes integrated out over S joint fantasies: row l of V is the Cholesky row that
// turns the innovation eps[s][l] of pick l into a shift of every candidate's mean, so under fantasy s
//     m_s(n) = (bias + p_n) + sum_{l<j} V[l][n] eps[s][l]        val_n = (1 / S) sum_s acq(m_s(n), s2_n, t_s)
// with the believer's own q' and s2 (the same in every fantasy).  k_fant_score is k_batch_score's frame around that value;
// k_fant_pick is k_batch_pick plus the fantasies' incumbents.  Per-candidate statements: acq_core.h (fant_*).
//
// eps (pick-major, pitch Sp: fant_ws) and t are wave-uniform: the round's j rows and t are copied to LDS once per workgroup
// (at most 63 x 64 + 64 doubles = 32 KB, dynamic) and every lane reads the same address (a broadcast).
// S is walked in chunks of FANT_CHUNK = 16 running means (32 VGPRs), the j rows of V walked again for every chunk: all 64 means
// live would cost 128 VGPRs on top of the EI evaluation, while the re-walked rows are j M doubles the fold has just pulled
// through L2 -- small beside the rank-1 pass's N M kernel evaluations per round (profiles/batch_fantasy.md).
// forced >= 0: the round's arg-max runs over that one row (a pending point); the fold runs over every candidate as always.
template <int ACQ>
__global__ __launch_bounds__(256) void k_fant_score(int j, int64_t M, const double* __restrict__ cq, const double* __restrict__ cp,
                                                    double* __restrict__ qp, double* __restrict__ V,
                                                    const double* __restrict__ cross, const double* __restrict__ scal,
                                                    const unsigned char* __restrict__ taken, double rho, double bias,
                                                    const double* __restrict__ eps, const double* __restrict__ tinc, int S, int Sp,
                                                    const int64_t* __restrict__ pend, int npend, double* __restrict__ s2_out,
                                                    double* __restrict__ partv, int64_t* __restrict__ parti) {
    extern __shared__ double fant_lds[];      // rows x Sp innovations, then Sp incumbents
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    const int rows = j + 1;                   // the picks made so far = the rows of V that shift the means
    double* const se = fant_lds;
    double* const st = fant_lds + rows * Sp;
    for (int i = threadIdx.x; i < rows * Sp; i += 256) se[i] = eps[i];
    for (int i = threadIdx.x; i < Sp; i += 256) st[i] = tinc[i];
    __syncthreads();
    const int64_t forced = (rows < npend) ? pend[rows] : -1;
    double bv = NEG_INF;
    int64_t bi = IDX_NONE;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < M; n += stride) {
        double q;
        if (j < 0) {
            q = cq[n];
        } else {
            q = batch_fold(j, M, n, V, cross, scal[1], V[(int64_t)j * M + n], qp[n]);
        }
        qp[n] = q;
        const CandMoments c = moments_of_sums(q, cp[n], rho, bias);
        if (s2_out) s2_out[n] = c.s2;
        if (taken[n] || (forced >= 0 && n != forced)) continue;
        double acc = 0.0;
        for (int c0 = 0; c0 < S; c0 += FANT_CHUNK) {
            double m[FANT_CHUNK];
#pragma unroll
            for (int k = 0; k < FANT_CHUNK; ++k) m[k] = c.mu;
            for (int l = 0; l < rows; ++l) {
                const double v = V[(int64_t)l * M + n];
                const double* e = se + l * Sp + c0;
#pragma unroll
                for (int k = 0; k < FANT_CHUNK; ++k) m[k] = fant_mean_step(m[k], v, e[k]);
            }
#pragma unroll
            for (int k = 0; k < FANT_CHUNK; ++k)
                if (c0 + k < S) fant_fold(c0 + k == 0, acq_value(ACQ, m[k], c.s2, st[c0 + k]), acc);
        }
        const double val = nan_last(fant_average(acc, S));
        if (better(val, n, bv, bi)) { bv = val; bi = n; }
    }
    block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        partv[blockIdx.x] = bv;
        parti[blockIdx.x] = bi;
    }
}

// k_batch_pick, then (update) one thread per fantasy moves its incumbent: t_s <- max(t_s, posterior mean at the pick after the
// fantasy's own observation there).  eps[j][s] is read, so the driver asks for no update after the last pick.
__global__ __launch_bounds__(256) void k_fant_pick(int j, int nblk, const double* __restrict__ partv,
                                                   const int64_t* __restrict__ parti, int64_t M, int d,
                                                   const double* __restrict__ Z, const double* __restrict__ invell,
                                                   const double* __restrict__ qp, const double* __restrict__ cp,
                                                   const double* __restrict__ V, double rho, double sn2, double bias,
                                                   const double* __restrict__ eps, double* __restrict__ tinc, int S, int Sp,
                                                   int update, double* __restrict__ x, double* __restrict__ xs,
                                                   double* __restrict__ scal, double* __restrict__ cross,
                                                   double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                   double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    const int64_t row = merge_pick(j, nblk, partv, parti, M, sel_val, sel_idx, taken);
    const int t = threadIdx.x;
    const double s2 = s2_floored(rho, qp[row]);
    if (t == 0) {
        sel_s2[j] = s2;
        pick_scalars(s2, sn2, scal);
    }
    if (t < j) cross[t] = V[(int64_t)t * M + row];
    for (int k = t; k < d; k += 256) {
        const double xv = Z[row * d + k];
        x[k] = xv;
        xs[k] = xv * invell[k];
    }
    if (update && t < S) {
        double sc[4];
        pick_scalars(s2, sn2, sc);
        tinc[t] = fant_incumbent(tinc[t], moments_of_sums(qp[row], cp[row], rho, bias).mu, j, V + row, M, eps + t, Sp, s2, sc[0]);
    }
}

// ---- the ensemble forms ---------------------------------------------------------------------------------------------------
// One thread per candidate, the members in order inside it.  HBM-bound, n (j + 4) 8 M bytes per round: member m + 1's three
// streaming loads (q', p, the raw row) are issued before member m's arithmetic, its cross-term rows follow as that retires.
__global__ __launch_bounds__(256) void k_ens_batch_score(int j, int nmem, int64_t M, const EnsBatchMember* __restrict__ mem,
                                                         const unsigned char* __restrict__ taken, int acq_id, double p0,
                                                         double* __restrict__ partv, int64_t* __restrict__ parti) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double bv = NEG_INF;
    int64_t bi = IDX_NONE;
    const int mode = (acq_id == GPX_ACQ_UCB) ? 1 : 0;
    const double nd = (double)nmem;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < M; n += stride) {
        double acc0 = 0.0, acc1 = 0.0;
        double qn = (j < 0) ? mem[0].cq[n] : mem[0].qp[n];
        double pn = mem[0].cp[n];
        double vn = (j < 0) ? 0.0 : mem[0].V[(int64_t)j * M + n];
        for (int m = 0; m < nmem; ++m) {
            const EnsBatchMember& e = mem[m];
            const double qprev = qn, p = pn, vraw = vn;
            if (m + 1 < nmem) {
                const EnsBatchMember& f = mem[m + 1];
                qn = (j < 0) ? f.cq[n] : f.qp[n];
                pn = f.cp[n];
                if (j >= 0) vn = f.V[(int64_t)j * M + n];
            }
            const double q = (j < 0) ? qprev : batch_fold(j, M, n, e.V, e.cross, e.scal[1], vraw, qprev);
            e.qp[n] = q;
            const CandMoments c = moments_of_sums(q, p, e.rho, e.bias);
            if (mode == 0)
                ens_fold(0, m == 0, acq_value(acq_id, c.mu, c.s2, p0), 0.0, acc0, acc1);
            else
                ens_fold(1, m == 0, c.mu, c.s2, acc0, acc1);
        }
        if (!taken[n]) {
            const double val = nan_last(ens_value(mode, acc0, acc1, nd, p0));
            if (better(val, n, bv, bi)) { bv = val; bi = n; }
        }
    }
    block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        partv[blockIdx.x] = bv;
        parti[blockIdx.x] = bi;
    }
}

// One workgroup.  Every member's scal: k_batch_pick's four words, from ITS conditioned variance at the pick.
__global__ __launch_bounds__(256) void k_ens_batch_pick(int j, int nblk, const double* __restrict__ partv,
                                                        const int64_t* __restrict__ parti, int64_t M, int d,
                                                        const double* __restrict__ Z, int nmem, int64_t nb,
                                                        const EnsBatchMember* __restrict__ mem, double* __restrict__ x,
                                                        double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                        double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    const int64_t row = merge_pick(j, nblk, partv, parti, M, sel_val, sel_idx, taken);
    const int t = threadIdx.x;
    for (int m = t; m < nmem; m += 256) {
        const EnsBatchMember& e = mem[m];
        const double s2 = s2_floored(e.rho, e.qp[row]);
        sel_s2[(int64_t)m * nb + j] = s2;
        pick_scalars(s2, e.sn2, e.scal);
    }
    for (int c = t; c < nmem * j; c += 256) {
        const int m = c / j, l = c - m * j;
        mem[m].cross[l] = mem[m].V[(int64_t)l * M + row];
    }
    for (int k = t; k < d; k += 256) {
        const double xv = Z[row * d + k];
        x[k] = xv;
        for (int m = 0; m < nmem; ++m) mem[m].xs[k] = xv * mem[m].invell[k];
    }
}

__global__ __launch_bounds__(256) void k_ens_same_grid(const unsigned long long* __restrict__ a,
                                                       const unsigned long long* __restrict__ b, int64_t words,
                                                       int* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    bool differ = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += stride) differ = differ || (a[i] != b[i]);
    if (differ) *flag = 1;
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

void launch_fant_score(hipStream_t s, int j, int64_t M, const double* cq, const double* cp, double* qp, double* V,
                       const double* cross, const double* scal, const unsigned char* taken, double rho, double bias, int acq_id,
                       const double* eps, const double* tinc, int S, int Sp, const int64_t* pend, int npend, double* s2_out,
                       double* partv, int64_t* parti) {
    const size_t lds = (size_t)(j + 2) * Sp * sizeof(double);      // j + 1 rows of innovations and the incumbents
    const dim3 grid((unsigned)batch_blocks(M));
    if (acq_id == GPX_ACQ_EI)
        hipLaunchKernelGGL(k_fant_score<GPX_ACQ_EI>, grid, dim3(256), lds, s, j, M, cq, cp, qp, V, cross, scal, taken, rho, bias,
                           eps, tinc, S, Sp, pend, npend, s2_out, partv, parti);
    else
        hipLaunchKernelGGL(k_fant_score<GPX_ACQ_PI>, grid, dim3(256), lds, s, j, M, cq, cp, qp, V, cross, scal, taken, rho, bias,
                           eps, tinc, S, Sp, pend, npend, s2_out, partv, parti);
}

void launch_fant_pick(hipStream_t s, int j, int64_t M, int d, const double* partv, const int64_t* parti, const double* Z,
                      const double* invell, const double* qp, const double* cp, const double* V, double rho, double sn2,
                      double bias, const double* eps, double* tinc, int S, int Sp, int update, double* x, double* xs, double* scal,
                      double* cross, double* sel_val, int64_t* sel_idx, double* sel_s2, unsigned char* taken) {
    hipLaunchKernelGGL(k_fant_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), partv, parti, M, d, Z, invell, qp, cp, V, rho,
                       sn2, bias, eps, tinc, S, Sp, update, x, xs, scal, cross, sel_val, sel_idx, sel_s2, taken);
}

void launch_ens_batch_score(hipStream_t s, int j, int n, int64_t M, const EnsBatchMember* mem, const unsigned char* taken,
                            int acq_id, double p0, double* partv, int64_t* parti) {
    hipLaunchKernelGGL(k_ens_batch_score, dim3((unsigned)batch_blocks(M)), dim3(256), 0, s, j, n, M, mem, taken, acq_id, p0,
                       partv, parti);
}

void launch_ens_batch_pick(hipStream_t s, int j, int n, int64_t nb, int64_t M, int d, const double* partv, const int64_t* parti,
                           const double* Z, const EnsBatchMember* mem, double* x, double* sel_val, int64_t* sel_idx,
                           double* sel_s2, unsigned char* taken) {
    hipLaunchKernelGGL(k_ens_batch_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), partv, parti, M, d, Z, n, nb, mem, x,
                       sel_val, sel_idx, sel_s2, taken);
}

void launch_ens_same_grid(hipStream_t s, const double* Za, const double* Zb, int64_t words, int* flag) {
    hipLaunchKernelGGL(k_ens_same_grid, dim3((unsigned)batch_blocks(words)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(Za), reinterpret_cast<const unsigned long long*>(Zb), words,
                       flag);
}

}  // namespace gpx
