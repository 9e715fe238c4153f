// kernels_batch.hip -- batch proposals (gpx_sweep_batch): nb greedy picks on the live sweep cache, each conditioned on the ones
// before it at their posterior mean (Kriging believer / GP-BUCB hallucination: the mean stays, the variance shrinks).
//
// With q' a scratch copy of the cache's q_n = |V(z_n)|^2, round j scores val_n = acq(bias + p_n, max(rho - q'_n, S2_FLOOR)), picks
// i_j = argmax over the candidates not picked yet (value descending, index ascending, NaN last: the top-k's order) and, unless
// it was the last pick, conditions on x = z_{i_j}:
//     c_n = k(x, z_n) - sum_i w_i k(x_i, z_n) - sum_{l<j} v_l[i_j] v_l[n]     w = K^-1 k(X, x)    d^2 = s2_{i_j} + sn2
//     v_j[n] = c_n / d        q'_n += v_j[n]^2
// The first two terms over d are one pass of the cache correction's rank-1 kernel (k_sweep_rankq<1> with `vout`, weight row
// [w, -1, 0..], xlast = x scaled) -- launched by the driver in api.hip between a round's two kernels.
//
// Five forms, ONE frame. A member's state is a BatchMember (acq_core.h); a scoring kernel is batch_score_frame (acq_core_dev.h: the
// walk over the candidates, who is live, the order, the block arg-max, the partial) around the one thing in which the forms differ, the
// value of a candidate; a pick kernel is merge_pick (the partials merged, the pick recorded), pick_member per member (its variance at
// the pick, 1/d, the cross terms v_l[i_j], x / ell) and pick_gather (the raw x), all in device scratch: the host never sees an index.
//   believer   gpx_sweep_batch           k_batch_score      acq_value at the member's moments                 k_batch_pick
//   fantasies  gpx_sweep_batch_fantasy   k_fant_score<ACQ>  the mean of acq_value over S fantasised means     k_fant_pick (+ incumbents)
//   ensemble   gpx_ensemble_sweep_batch  k_ens_batch_score  the members' values or moments folded in order    k_ens_batch_pick
//   constrained gpx_constrained_sweep_batch k_con_batch_score  the objective's value times every constraint's PI  k_ens_batch_pick
//   two objectives gpx_ehvi_sweep_batch   k_ehvi_batch_score EHVI of the two members' moments over the front's strips  k_ehvi_batch_pick (+ the front)
// The single-model kernels take their member by value, the ensemble's and the constrained form's read a table of n in device memory: every member is conditioned
// on the pick at ITS OWN posterior mean and keeps its own w, d, cross terms, 1/ell, V and q'.  k_ens_same_grid: the members' caches hold
// the same candidates, bit for bit (one flag word, read at the call's only sync).
// The argmax runs over a total order and every candidate's arithmetic is its own thread's: results do not depend on the grid.
// Per-candidate statements (the order, the moments, batch_cand / batch_fold, a pick's scalars, the ensemble's fold and finish, fant_*)
// are acq_core.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acq_core_dev.h"
#include "gpx_internal.h"
#include "gpx_math.h"
#define GPX_EHVI_DEVICE
#include "ehvi_math.h"

namespace gpx {

// j < 0: round 0.  j >= 0: row j of V holds the rank-1 pass's (k(x, z_n) - w . k(X, z_n)) / d, folded by batch_cand.
__global__ __launch_bounds__(256) void k_batch_score(int j, int64_t M, BatchMember e, const unsigned char* __restrict__ taken, int acq_id,
                                                     double p0, double* __restrict__ s2_out, double* __restrict__ partv,
                                                     int64_t* __restrict__ parti) {
    batch_score_frame(M, taken, -1, [&](int64_t n) { return batch_cand(j, M, n, e, s2_out); },
                      [&](int64_t, const CandMoments& c) { return acq_value(acq_id, c.mu, c.s2, p0); }, partv, parti);
}

// The believer's recurrence with the pending outcomes integrated out over S joint fantasies: row l of V is the Cholesky row that
// turns the innovation eps[s][l] of pick l into a shift of every candidate's mean, so under fantasy s
//     m_s(n) = (bias + p_n) + sum_{l<j} V[l][n] eps[s][l]        val_n = (1 / S) sum_s acq(m_s(n), s2_n, t_s)
// with the believer's own q' and s2 (the same in every fantasy).
// eps (pick-major, pitch Sp: fant_ws) and t are wave-uniform: the round's j rows and t are copied to LDS once per workgroup
// (at most 63 x 64 + 64 doubles = 32 KB, dynamic) and every lane reads the same address (a broadcast).
// S is walked in chunks of FANT_CHUNK = 16 running means (32 VGPRs), the j rows of V walked again for every chunk: all 64 means
// live would cost 128 VGPRs on top of the EI evaluation, while the re-walked rows are j M doubles the fold has just pulled
// through L2 -- small beside the rank-1 pass's N M kernel evaluations per round (profiles/batch_fantasy.md).
// A round forced to a pending row scores that one row; the fold runs over every candidate as always.
template <int ACQ>
__global__ __launch_bounds__(256) void k_fant_score(int j, int64_t M, BatchMember e, const unsigned char* __restrict__ taken, FantArg f,
                                                    double* __restrict__ s2_out, double* __restrict__ partv,
                                                    int64_t* __restrict__ parti) {
    extern __shared__ double fant_lds[];      // rows x Sp innovations, then Sp incumbents
    const int rows = j + 1;                   // the picks made so far = the rows of V that shift the means
    const int S = f.S, Sp = f.Sp;
    double* const se = fant_lds;
    double* const st = fant_lds + rows * Sp;
    for (int i = threadIdx.x; i < rows * Sp; i += 256) se[i] = f.eps[i];
    for (int i = threadIdx.x; i < Sp; i += 256) st[i] = f.t[i];
    __syncthreads();
    const auto fold = [&](int64_t n) { return batch_cand(j, M, n, e, s2_out); };
    batch_score_frame(M, taken, (rows < f.npend) ? f.pend[rows] : -1, fold, [&](int64_t n, const CandMoments& c) {
        double acc = 0.0;
        for (int c0 = 0; c0 < S; c0 += FANT_CHUNK) {
            double m[FANT_CHUNK];
#pragma unroll
            for (int k = 0; k < FANT_CHUNK; ++k) m[k] = c.mu;
            for (int l = 0; l < rows; ++l) {
                const double v = e.V[(int64_t)l * M + n];
                const double* ep = se + l * Sp + c0;
#pragma unroll
                for (int k = 0; k < FANT_CHUNK; ++k) m[k] = fant_mean_step(m[k], v, ep[k]);
            }
#pragma unroll
            for (int k = 0; k < FANT_CHUNK; ++k)
                if (c0 + k < S) fant_fold(c0 + k == 0, acq_value(ACQ, m[k], c.s2, st[c0 + k]), acc);
        }
        return fant_average(acc, S);
    }, partv, parti);
}

// One thread per candidate, the members in order inside it.  HBM-bound, n (j + 4) 8 M bytes per round: member m + 1's three
// streaming loads (q', p, the raw row) are issued before member m's arithmetic, its cross-term rows follow as that retires.
__global__ __launch_bounds__(256) void k_ens_batch_score(int j, int nmem, int64_t M, const BatchMember* __restrict__ mem,
                                                         const unsigned char* __restrict__ taken, int acq_id, double p0,
                                                         double* __restrict__ partv, int64_t* __restrict__ parti) {
    const int mode = (acq_id == GPX_ACQ_UCB) ? 1 : 0;
    const double nd = (double)nmem;
    struct Sums { double acc0, acc1; };
    const auto fold = [&](int64_t n) {
        double acc0 = 0.0, acc1 = 0.0;
        double qn = (j < 0) ? mem[0].cq[n] : mem[0].qp[n];
        double pn = mem[0].cp[n];
        double vn = (j < 0) ? 0.0 : mem[0].V[(int64_t)j * M + n];
        for (int m = 0; m < nmem; ++m) {
            const BatchMember& e = mem[m];
            const double qprev = qn, p = pn, vraw = vn;
            if (m + 1 < nmem) {
                const BatchMember& f = mem[m + 1];
                qn = (j < 0) ? f.cq[n] : f.qp[n];
                pn = f.cp[n];
                if (j >= 0) vn = f.V[(int64_t)j * M + n];
            }
            const CandMoments c = moments_of_sums(batch_q(j, M, n, e.V, e.cross, e.scal, e.qp, qprev, vraw), p, e.rho, e.bias);
            if (mode == 0)
                ens_fold(0, m == 0, acq_value(acq_id, c.mu, c.s2, p0), 0.0, acc0, acc1);
            else
                ens_fold(1, m == 0, c.mu, c.s2, acc0, acc1);
        }
        return Sums{acc0, acc1};
    };
    batch_score_frame(M, taken, -1, fold, [&](int64_t, const Sums& a) { return ens_value(mode, a.acc0, a.acc1, nd, p0); }, partv, parti);
}

// Two objectives (a table of two members): each member's own recurrence and moments on the load schedule above -- objective 2's three
// streaming loads are issued before objective 1's arithmetic --, then ehvi_value over the strips of the front AS THE DEVICE HOLDS IT:
// *n_word points (the pick kernel moves it), a then b of pitch EHVI_STRIP_LD, staged once per workgroup into LDS as in k_ehvi_fold; in
// the loop every lane reads the same word, which the LDS broadcasts.  Compute-bound from a few strips on: 2 (n + 1) + 1 EI per candidate.
__global__ __launch_bounds__(256) void k_ehvi_batch_score(int j, int64_t M, const BatchMember* __restrict__ mem,
                                                          const unsigned char* __restrict__ taken, const double* __restrict__ strips,
                                                          const int* __restrict__ n_word, double* __restrict__ partv,
                                                          int64_t* __restrict__ parti) {
    __shared__ double sa[EHVI_STRIP_LD], sb[EHVI_STRIP_LD];
    const int nf = min(max(*n_word, 0), EHVI_MAX_FRONT);      // (the driver's capacity rule keeps it there; never index past the arrays)
    for (int i = threadIdx.x; i < nf + 2; i += 256) {
        sa[i] = strips[i];
        sb[i] = strips[EHVI_STRIP_LD + i];
    }
    __syncthreads();
    struct Mom { double mu1, s2_1, mu2, s2_2; };
    const auto fold = [&](int64_t n) {
        const BatchMember& e = mem[0];
        const BatchMember& f = mem[1];
        const double q1 = (j < 0) ? e.cq[n] : e.qp[n], p1 = e.cp[n], v1 = (j < 0) ? 0.0 : e.V[(int64_t)j * M + n];
        const double q2 = (j < 0) ? f.cq[n] : f.qp[n], p2 = f.cp[n], v2 = (j < 0) ? 0.0 : f.V[(int64_t)j * M + n];
        const CandMoments c1 = moments_of_sums(batch_q(j, M, n, e.V, e.cross, e.scal, e.qp, q1, v1), p1, e.rho, e.bias);
        const CandMoments c2 = moments_of_sums(batch_q(j, M, n, f.V, f.cross, f.scal, f.qp, q2, v2), p2, f.rho, f.bias);
        return Mom{c1.mu, c1.s2, c2.mu, c2.s2};
    };
    batch_score_frame(M, taken, -1, fold, [&](int64_t, const Mom& c) { return ehvi_value(c.mu1, c.s2_1, c.mu2, c.s2_2, sa, sb, nf); },
                      partv, parti);
}

// The constrained index over the same table (the objective first where a.has_obj, then the constraints in the caller's order): every
// member's own recurrence and moments as above, its term -- acq_value of the objective at the target, PI of a constraint at its
// threshold -- taken into the chain by con_chain.  The same load schedule, the same n (j + 4) 8 M bytes per round.
__global__ __launch_bounds__(256) void k_con_batch_score(int j, int nmem, int64_t M, const BatchMember* __restrict__ mem,
                                                         const unsigned char* __restrict__ taken, ConBatchArg a,
                                                         double* __restrict__ partv, int64_t* __restrict__ parti) {
    const auto fold = [&](int64_t n) {
        double v = 0.0;
        double qn = (j < 0) ? mem[0].cq[n] : mem[0].qp[n];
        double pn = mem[0].cp[n];
        double vn = (j < 0) ? 0.0 : mem[0].V[(int64_t)j * M + n];
        for (int m = 0; m < nmem; ++m) {
            const BatchMember& e = mem[m];
            const double qprev = qn, p = pn, vraw = vn;
            if (m + 1 < nmem) {
                const BatchMember& f = mem[m + 1];
                qn = (j < 0) ? f.cq[n] : f.qp[n];
                pn = f.cp[n];
                if (j >= 0) vn = f.V[(int64_t)j * M + n];
            }
            const CandMoments c = moments_of_sums(batch_q(j, M, n, e.V, e.cross, e.scal, e.qp, qprev, vraw), p, e.rho, e.bias);
            const bool objective = m < a.has_obj;
            v = con_chain(m == 0, objective, v,
                          acq_value(objective ? a.acq_id : GPX_ACQ_PI, c.mu, c.s2, objective ? a.target : a.thr[m - a.has_obj]));
        }
        return v;
    };
    batch_score_frame(M, taken, -1, fold, [&](int64_t, double v) { return v; }, partv, parti);
}

// The single-model pick (one workgroup).  f.S > 0: one thread per fantasy then moves its incumbent, t_s <- max(t_s, posterior mean at
// the pick after the fantasy's own observation there); eps[j][s] is read, so the driver passes no fantasies after the last pick.
__device__ __forceinline__ void single_pick(int j, int nblk, const double* __restrict__ partv, const int64_t* __restrict__ parti, int64_t M,
                                            int d, const double* __restrict__ Z, const BatchMember& e, const FantArg& f,
                                            double* __restrict__ x, double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                            double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    const int64_t row = merge_pick(j, nblk, partv, parti, M, sel_val, sel_idx, taken);
    const int t = threadIdx.x;
    const double s2 = pick_member(e, j, M, d, Z, row, sel_s2, t, 256);
    pick_gather(Z, row, d, x);
    if (t < f.S) {
        double sc[4];
        pick_scalars(s2, e.sn2, sc);
        f.t[t] = fant_incumbent(f.t[t], moments_of_sums(e.qp[row], e.cp[row], e.rho, e.bias).mu, j, e.V + row, M, f.eps + t, f.Sp, s2, sc[0]);
    }
}

__global__ __launch_bounds__(256) void k_batch_pick(int j, int nblk, const double* __restrict__ partv, const int64_t* __restrict__ parti,
                                                    int64_t M, int d, const double* __restrict__ Z, BatchMember e, double* __restrict__ x,
                                                    double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                    double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    single_pick(j, nblk, partv, parti, M, d, Z, e, FantArg(), x, sel_val, sel_idx, sel_s2, taken);
}

__global__ __launch_bounds__(256) void k_fant_pick(int j, int nblk, const double* __restrict__ partv, const int64_t* __restrict__ parti,
                                                   int64_t M, int d, const double* __restrict__ Z, BatchMember e, FantArg f,
                                                   double* __restrict__ x, double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                   double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    single_pick(j, nblk, partv, parti, M, d, Z, e, f, x, sel_val, sel_idx, sel_s2, taken);
}

// One workgroup, a wave per member (four at a time; j < 64 lanes hold a member's cross terms).  sel_s2: (nmem, nb) member-major.
__global__ __launch_bounds__(256) void k_ens_batch_pick(int j, int nblk, const double* __restrict__ partv,
                                                        const int64_t* __restrict__ parti, int64_t M, int d,
                                                        const double* __restrict__ Z, int nmem, int64_t nb,
                                                        const BatchMember* __restrict__ mem, double* __restrict__ x,
                                                        double* __restrict__ sel_val, int64_t* __restrict__ sel_idx,
                                                        double* __restrict__ sel_s2, unsigned char* __restrict__ taken) {
    const int64_t row = merge_pick(j, nblk, partv, parti, M, sel_val, sel_idx, taken);
    for (int m = threadIdx.x >> 6; m < nmem; m += 4) pick_member(mem[m], j, M, d, Z, row, sel_s2 + (int64_t)m * nb, threadIdx.x & 63, 64);
    pick_gather(Z, row, d, x);
}

// k_ens_batch_pick for the two objectives, and the front follows the pick: one thread records the size of the front that scored pick j and
// the believed outcome y_j -- each member's own posterior mean bias + p[row], which the believer does not move -- and, unless it was the
// last pick, takes y_j into the strips by ehvi_insert (the host's text; at most n + 2 words move, in place).  The next scoring pass reads
// the strips and *w.n: neither the index nor the front's size reaches the host before the call's final copy.
__global__ __launch_bounds__(256) void k_ehvi_batch_pick(int j, int nblk, const double* __restrict__ partv,
                                                         const int64_t* __restrict__ parti, int64_t M, int d,
                                                         const double* __restrict__ Z, int64_t nb, const BatchMember* __restrict__ mem,
                                                         double* __restrict__ x, double* __restrict__ sel_val,
                                                         int64_t* __restrict__ sel_idx, double* __restrict__ sel_s2,
                                                         unsigned char* __restrict__ taken, EhviBatchWs w, int last) {
    const int64_t row = merge_pick(j, nblk, partv, parti, M, sel_val, sel_idx, taken);
    for (int m = threadIdx.x >> 6; m < 2; m += 4) pick_member(mem[m], j, M, d, Z, row, sel_s2 + (int64_t)m * nb, threadIdx.x & 63, 64);
    pick_gather(Z, row, d, x);
    if (threadIdx.x == 0) {
        const int n = *w.n;
        const double y1 = moments_of_sums(mem[0].qp[row], mem[0].cp[row], mem[0].rho, mem[0].bias).mu;
        const double y2 = moments_of_sums(mem[1].qp[row], mem[1].cp[row], mem[1].rho, mem[1].bias).mu;
        w.nfront[j] = n;
        w.y[2 * j] = y1;
        w.y[2 * j + 1] = y2;
        if (!last && n >= 0 && n < EHVI_MAX_FRONT) *w.n = ehvi_insert(w.a, w.b, n, y1, y2);      // (n < the cap: the driver's capacity rule)
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

void launch_batch_score(hipStream_t s, int j, int64_t M, const BatchMember& e, const BatchBuf& b, int acq_id, double p0, const FantArg* f,
                        double* s2_out) {
    const dim3 grid((unsigned)batch_blocks(M));
    if (!f) {
        hipLaunchKernelGGL(k_batch_score, grid, dim3(256), 0, s, j, M, e, b.taken, acq_id, p0, s2_out, b.partv, b.parti);
        return;
    }
    const size_t lds = (size_t)(j + 2) * f->Sp * sizeof(double);      // j + 1 rows of innovations and the incumbents
    if (acq_id == GPX_ACQ_EI)
        hipLaunchKernelGGL(k_fant_score<GPX_ACQ_EI>, grid, dim3(256), lds, s, j, M, e, b.taken, *f, s2_out, b.partv, b.parti);
    else
        hipLaunchKernelGGL(k_fant_score<GPX_ACQ_PI>, grid, dim3(256), lds, s, j, M, e, b.taken, *f, s2_out, b.partv, b.parti);
}

void launch_batch_pick(hipStream_t s, int j, int64_t M, int d, const double* Z, const BatchMember& e, const BatchBuf& b, const FantArg* f,
                       bool update) {
    if (!f) {
        hipLaunchKernelGGL(k_batch_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), b.partv, b.parti, M, d, Z, e, b.x, b.sel_val, b.sel_idx,
                           b.sel_s2, b.taken);
        return;
    }
    FantArg g = *f;
    if (!update) g.S = 0;
    hipLaunchKernelGGL(k_fant_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), b.partv, b.parti, M, d, Z, e, g, b.x, b.sel_val, b.sel_idx,
                       b.sel_s2, b.taken);
}

void launch_ens_batch_score(hipStream_t s, int j, int n, int64_t M, const BatchMember* mem, const BatchBuf& b, int acq_id, double p0) {
    hipLaunchKernelGGL(k_ens_batch_score, dim3((unsigned)batch_blocks(M)), dim3(256), 0, s, j, n, M, mem, b.taken, acq_id, p0, b.partv,
                       b.parti);
}

void launch_con_batch_score(hipStream_t s, int j, int n, int64_t M, const BatchMember* mem, const BatchBuf& b, const ConBatchArg& a) {
    hipLaunchKernelGGL(k_con_batch_score, dim3((unsigned)batch_blocks(M)), dim3(256), 0, s, j, n, M, mem, b.taken, a, b.partv, b.parti);
}

void launch_ehvi_batch_score(hipStream_t s, int j, int64_t M, const BatchMember* mem, const BatchBuf& b, const EhviBatchWs& w) {
    hipLaunchKernelGGL(k_ehvi_batch_score, dim3((unsigned)batch_blocks(M)), dim3(256), 0, s, j, M, mem, b.taken, w.a, w.n, b.partv, b.parti);
}

void launch_ehvi_batch_pick(hipStream_t s, int j, int64_t nb, int64_t M, int d, const double* Z, const BatchMember* mem, const BatchBuf& b,
                            const EhviBatchWs& w, bool last) {
    hipLaunchKernelGGL(k_ehvi_batch_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), b.partv, b.parti, M, d, Z, nb, mem, b.x, b.sel_val,
                       b.sel_idx, b.ens_s2, b.taken, w, last ? 1 : 0);
}

void launch_ens_batch_pick(hipStream_t s, int j, int n, int64_t nb, int64_t M, int d, const double* Z, const BatchMember* mem,
                           const BatchBuf& b) {
    hipLaunchKernelGGL(k_ens_batch_pick, dim3(1), dim3(256), 0, s, j, batch_blocks(M), b.partv, b.parti, M, d, Z, n, nb, mem, b.x, b.sel_val,
                       b.sel_idx, b.ens_s2, b.taken);
}

void launch_ens_same_grid(hipStream_t s, const double* Za, const double* Zb, int64_t words, int* flag) {
    hipLaunchKernelGGL(k_ens_same_grid, dim3((unsigned)batch_blocks(words)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(Za), reinterpret_cast<const unsigned long long*>(Zb), words,
                       flag);
}

}  // namespace gpx
