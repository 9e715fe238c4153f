// acq_core.h -- the per-candidate arithmetic every acquisition kernel shares, each piece defined ONCE: the sums and moments of a
// candidate, the variance floor, the ensemble's fold and finish, the constraint fold and chain, the total order of the top-k and of the batch picks, a batch member's state and its
// fold, a pick's four scalars and the fantasised picks' mean step, average and incumbent.  The library promises bit-for-bit agreement between many of its paths (a cache seeded by any
// acquisition, pruned against exhaustive sweeps, ensemble against its members, batch against single picks); those promises hold
// because the paths call the functions below, not because their statements were kept in step.
// Plain C++ (no HIP type, no thread index): the kernels and the host-only program tests/c/acq_core_check.cpp include this one
// file, so the host checks the statements the device runs.  What needs a workgroup (the arg-max reduction, the frames of the
// acquisition and pick kernels) is in acq_core_dev.h; acq_value stays in gpx_math.h (the device library's erfc / exp).
// Nothing here may be re-associated, fused or replaced by an intrinsic: the functions whose results are compared with host
// arithmetic carry `fp contract(off)` themselves (GPX_NO_CONTRACT), whatever the including file compiles under.
#ifndef GPX_ACQ_CORE_H
#define GPX_ACQ_CORE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPX_ACQ_FN __host__ __device__ __forceinline__
#else
#define GPX_ACQ_FN inline
#endif
// first statement of a function whose multiplies and adds must each round (no FMA contraction), whatever the including file compiles
// under; a host compiler that does not know the pragma builds with -ffp-contract=off instead
#if defined(__clang__)
#define GPX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GPX_NO_CONTRACT
#endif

namespace gpx {

// ---- sums and moments ---------------------------------------------------------------------------------------------------------
// The posterior variance is never reported below this (rho - q cancels to rounding noise, or below 0, on top of an observation).
// The host's legality tests of the pruned sweeps (api.hip: rho >= S2_FLOOR) are its twin.
constexpr double S2_FLOOR = 1e-100;

struct CandMoments {
    double q, p;      // |V(z)|^2 and V(z)^T a: what a sweep cache keeps
    double mu, s2;
};

// adds column n of the per-row-block partials (nrb, ldp) onto q (and p, WITH_P), the blocks in ascending order
template <bool WITH_P>
GPX_ACQ_FN void add_rowblocks(const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t n, double& q, double& p) {
    for (int rb = 0; rb < nrb; ++rb) {
        q += Qp[(int64_t)rb * ldp + n];
        if (WITH_P) p += Pp[(int64_t)rb * ldp + n];
    }
}

GPX_ACQ_FN double s2_floored(double rho, double q) { return fmax(rho - q, S2_FLOOR); }      // (q NaN: the floor)

GPX_ACQ_FN CandMoments moments_of_sums(double q, double p, double rho, double bias) { return {q, p, bias + p, s2_floored(rho, q)}; }

// nrb > 0: Qp/Pp are per-row-block partials, reduced here.  nrb = 0: they are the already reduced sums (the sweep cache).
GPX_ACQ_FN CandMoments cand_moments(const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t n, double rho, double bias) {
    double q = 0.0, p = 0.0;
    if (nrb == 0) {
        q = Qp[n];
        p = Pp[n];
    }
    add_rowblocks<true>(Qp, Pp, ldp, nrb, n, q, p);
    return moments_of_sums(q, p, rho, bias);
}

// ---- the ensemble ---------------------------------------------------------------------------------------------------------------
// One addition per member in member order, then ONE division by n: the association of numpy's mean over axis 0.
//   mode 0 (EI / PI / mean / MES):  acc0 += t0
//   mode 1 (UCB, mixture moments):  acc0 += mu_m;  acc1 += s2_m + mu_m^2        (t0 = mu_m, t1 = s2_m)
// mode 0 leaves acc1 alone; `first` starts the sums at the member's terms, whatever acc0 / acc1 held.
GPX_ACQ_FN void ens_fold(int mode, bool first, double t0, double t1, double& acc0, double& acc1) {
    GPX_NO_CONTRACT;
    if (mode == 0) {
        acc0 = first ? t0 : acc0 + t0;
    } else {
        const double m2 = t0 * t0;
        const double q = t1 + m2;
        acc0 = first ? t0 : acc0 + t0;
        acc1 = first ? q : acc1 + q;
    }
}

GPX_ACQ_FN double ens_mean(double acc0, double n) {
    GPX_NO_CONTRACT;
    return acc0 / n;
}

// the mixture's variance: mu^2 rounded before the subtraction; one member gives fl(fl(s2 + mu^2) - mu^2), NOT s2
GPX_ACQ_FN double ens_mix_s2(double mu, double acc1, double n) {
    GPX_NO_CONTRACT;
    const double mu2 = mu * mu;
    double s2 = acc1 / n - mu2;
    s2 = fmax(s2, 0.0);
    return s2;
}

GPX_ACQ_FN double ens_ucb(double mu, double s2, double beta) {
    GPX_NO_CONTRACT;
    return mu + sqrt(beta * s2);
}

GPX_ACQ_FN double ens_value(int mode, double acc0, double acc1, double n, double beta) {
    const double mu = ens_mean(acc0, n);
    if (mode == 0) return mu;
    return ens_ucb(mu, ens_mix_s2(mu, acc1, n), beta);
}

// ---- constraints ------------------------------------------------------------------------------------------------------------------
// One factor of a constrained index (gpx_constrained_sweep): v_j = con_fold(v_{j-1}, P_j), P_j a probability of feasibility.  The clamp
// makes 0 <= factor <= 1 a property of this function, not of the device's erfc, so that fl(v * factor) <= v for every v >= 0: a bound on
// the objective's value is a bound on the product, bit for bit.  A NaN p stays NaN (the comparison is false).
GPX_ACQ_FN double con_fold(double v, double p) {
    GPX_NO_CONTRACT;
    return v * (p > 1.0 ? 1.0 : p);
}

// The chain of a constrained index one member at a time (gpx_constrained_sweep_batch: the members in the caller's order, the objective
// first where there is one): t is the member's own term -- the objective's EI / PI, a constraint's probability of feasibility -- and v the
// chain so far, unread by the first member.  The objective starts the chain at its value; without one the first constraint starts it
// at con_fold(1, P_1), exactly as k_con_fold starts pof_all.
GPX_ACQ_FN double con_chain(bool first, bool objective, double v, double t) {
    GPX_NO_CONTRACT;
    if (objective) return t;
    return con_fold(first ? 1.0 : v, t);
}

// what the constrained batch's scoring kernel takes by value: the thresholds in constraint order, the objective's target and acquisition
struct ConBatchArg {
    double thr[16];
    double target;
    int acq_id, has_obj;      // has_obj 1: member 0 is the objective, constraint j is member 1 + j; 0: constraint j is member j
};

// ---- the order --------------------------------------------------------------------------------------------------------------------
// value descending, ties -> lower index, NaN below everything: a strict total order on (nan_last(value), index)
constexpr double NEG_INF = -__builtin_huge_val();
constexpr int64_t IDX_NONE = 0x7fffffffffffffffLL;      // no candidate: ranks after every index at NEG_INF

GPX_ACQ_FN bool better(double av, int64_t ai, double bv, int64_t bi) { return (av > bv) || (av == bv && ai < bi); }

GPX_ACQ_FN double nan_last(double v) { return (v != v) ? NEG_INF : v; }

// ---- batch picks ------------------------------------------------------------------------------------------------------------------
// The fold of round j >= 0: vraw = V[j][n] as the rank-1 pass left it, qprev = q'_n.  The cross terms are taken off in pick order,
// each product rounded before it is added, then divided once by d.  Stores v_j[n], returns the new q'_n.
GPX_ACQ_FN double batch_fold(int j, int64_t M, int64_t n, double* __restrict__ V, const double* __restrict__ cross, double invd,
                             double vraw, double qprev) {
    GPX_NO_CONTRACT;
    double t = 0.0;
    for (int l = 0; l < j; ++l) {
        const double prod = cross[l] * V[(int64_t)l * M + n];
        t = t + prod;
    }
    const double td = t * invd;
    const double v = vraw - td;
    V[(int64_t)j * M + n] = v;
    const double vv = v * v;
    return qprev + vv;
}

// One member's batch state as every kernel of kernels_batch.hip sees it (gpx_sweep_batch and gpx_sweep_batch_fantasy: the one model,
// by value; gpx_ensemble_sweep_batch: a table of n in device memory): the member's cached sums, its model constants, and where its
// recurrence lies in its own handle's dbsel (batch_ws).  What a batch shares -- the candidates, the raw x, taken, the partials, the
// picks -- belongs to the lead and travels beside it.
struct BatchMember {
    const double *cq, *cp, *invell;
    double *qp, *V, *cross, *scal, *xs;
    double rho, bias, sn2;
};

// what the fantasised form adds (fant_ws): the innovations pick-major with pitch Sp, the S incumbents, the forced rows of the leading rounds
struct FantArg {
    const double* eps;
    double* t;
    const int64_t* pend;
    int S, Sp, npend;
};

// Member e's q' of candidate n in the round after pick j (j < 0: round 0, q' <- q of the cache), stored and returned, from its streamed
// words qprev (q, else q') and vraw (row j of V as the rank-1 pass left it; unread in round 0)
// (a member's pointers are taken apart into __restrict__ parameters here: a struct's fields cannot promise that they do not alias,
// and without the promise the scoring kernels hold two to twenty-six more VGPRs and lose a wave per SIMD)
GPX_ACQ_FN double batch_q(int j, int64_t M, int64_t n, double* __restrict__ V, const double* __restrict__ cross, const double* __restrict__ scal,
                          double* __restrict__ qp, double qprev, double vraw) {
    const double q = (j < 0) ? qprev : batch_fold(j, M, n, V, cross, scal[1], vraw, qprev);
    qp[n] = q;
    return q;
}

// the single-model forms' candidate: its words loaded here, its moments, the optional store of the variance
GPX_ACQ_FN CandMoments batch_cand(int j, int64_t M, int64_t n, const double* __restrict__ cq, const double* __restrict__ cp, double* __restrict__ qp,
                                  double* __restrict__ V, const double* __restrict__ cross, const double* __restrict__ scal, double rho,
                                  double bias, double* __restrict__ s2_out) {
    const double q = (j < 0) ? batch_q(j, M, n, V, cross, scal, qp, cq[n], 0.0)      // (one branch on j, not a select per word)
                             : batch_q(j, M, n, V, cross, scal, qp, qp[n], V[(int64_t)j * M + n]);
    const CandMoments c = moments_of_sums(q, cp[n], rho, bias);
    if (s2_out) s2_out[n] = c.s2;
    return c;
}
GPX_ACQ_FN CandMoments batch_cand(int j, int64_t M, int64_t n, const BatchMember& e, double* s2_out) {
    return batch_cand(j, M, n, e.cq, e.cp, e.qp, e.V, e.cross, e.scal, e.rho, e.bias, s2_out);
}

// a pick's four scalars from its conditioned variance: [0] d  [1] 1/d  [2] 0 (the `a` slot of launch_pend_store: no value exists)  [3] d^2
GPX_ACQ_FN void pick_scalars(double s2, double sn2, double* scal) {
    const double d2 = s2 + sn2;
    const double dd = sqrt(d2);
    scal[0] = dd;
    scal[1] = 1.0 / dd;
    scal[2] = 0.0;
    scal[3] = d2;
}

// ---- fantasised batch picks ---------------------------------------------------------------------------------------------------
// Pending observations integrated out over S joint fantasies (gpx_sweep_batch_fantasy): row l of V turns the standard-normal
// innovation eps[s][l] of pick l into a shift of every candidate's mean.  One step of a fantasy's mean, the product rounded before
// it is added; the walk starts at bias + p (moments_of_sums' mu) and takes the rows in pick order.  A zero eps leaves mu's bits.
GPX_ACQ_FN double fant_mean_step(double m, double v, double e) {
    GPX_NO_CONTRACT;
    const double prod = v * e;
    return m + prod;
}

// the fantasy average of S values: ens_fold's mode 0 in fantasy order (`first` starts the sum at the term), then ens_mean's one
// division (S = 1: the value's own bits)
GPX_ACQ_FN void fant_fold(bool first, double val, double& acc) {
    double unused = 0.0;
    ens_fold(0, first, val, 0.0, acc, unused);
}

GPX_ACQ_FN double fant_average(double acc, int S) { return ens_mean(acc, (double)S); }

// A fantasy's incumbent after pick j at row r: its posterior mean at the pick right after its own fantasised observation there,
//     u = (bias + p_r) + sum_{i<j} V[i][r] eps[i] + (s2 / d) eps[j]          t <- max(t, u)
// mu = bias + p_r; cross[i * cs] = V[i][r] (cs = 1: the gathered cross terms, cs = M: the rows of V at column r); eps: the fantasy's
// innovations with stride es; s2, d: the pick's conditioned variance and pick_scalars' d.  A NaN u leaves t.
GPX_ACQ_FN double fant_incumbent(double t, double mu, int j, const double* cross, int64_t cs, const double* eps, int64_t es, double s2,
                                 double d) {
    GPX_NO_CONTRACT;
    double u = mu;
    for (int i = 0; i < j; ++i) u = fant_mean_step(u, cross[(int64_t)i * cs], eps[(int64_t)i * es]);
    const double gain = s2 / d;
    u = fant_mean_step(u, gain, eps[(int64_t)j * es]);
    return fmax(t, u);
}

}  // namespace gpx

#endif
