// kg_math.h -- the knowledge gradient of a finite set of lines (Frazier, Powell & Dayanik 2009):
//     KG = E_Z[max_j (a_j + b_j Z)] - max_j a_j >= 0,   Z ~ N(0, 1),   j = 0 .. n - 1,   n <= KG_MAX_LINES.
// Plain C++ (templates over a line accessor with .a(i), .b(i)); the kernels of kernels_kg.hip and the host-only program
// tests/c/kg_math_check.cpp include this one file, so the host checks the statements the device runs (the two sides differ only in
// their libraries' exp and erfc, which the bound below charges).
//
// FORM.  Line j is the upper envelope on (lo_j, hi_j): lo_j = max over the flatter lines i of the crossing c_ij = (a_i - a_j) / (b_j - b_i),
// hi_j = min over the steeper ones of the same expression; among lines of equal slope only the largest intercept counts, the lowest
// index on a tie (the others are off).  Frazier's sum over the envelope's crossings, sum_i (b_(i+1) - b_(i)) H(c_i) with
// H(c) = h(-|c|), h(c) = phi(c) + c Phi(c), regrouped per LINE (every crossing is the hi of its left line and the lo of its right one):
//     KG = sum_{j on} (b_j - b_ref) (H(lo_j) - H(hi_j)),      H(+-inf) = 0,
// where b_ref is any constant, because sum_{j on} (H(lo_j) - H(hi_j)) telescopes to 0; b_ref = b_0 here.  No sort, no "next line":
// a line's term needs its own interval only, so a line whose interval is empty to rounding (three nearly concurrent lines)
// contributes (b_j - b_0) (H(lo) - H(hi)) ~ 0 whether it is judged on or off -- the sum is continuous across that decision.
// The n terms are summed in KG_WAYS interleaved partial sums (lines j = t, t + KG_WAYS, ..; ((p_0 + p_1) + p_2) + p_3): the order
// is a function of the line indices alone, on the host and in every thread layout of the device.
//
// h.  x = |c|.  x < 8: h(-x) = phi(x) - x Q(x), Q = erfc(x / sqrt 2) / 2.  phi = exp(-x^2 / 2) with the rounding of x^2 put back by one
// FMA (3 eps with a 1-ulp exp); Q: the argument x / sqrt 2 carries 1.5 eps, which erfc's logarithmic derivative (<= x^2 + 1) turns into
// 1.5 (x^2 + 1) eps, plus <= 4 eps of the library's erfc and 1 eps of the product: (1.5 x^2 + 6.5) eps.  The difference cancels:
// h(-x) / phi(x) = 1 - x R(x) >= 1 / (x^2 + 3) (R Mills' ratio, R <= (x^2 + 2) / (x (x^2 + 3))), so both terms are at most (x^2 + 3) h and
//     |dh| / h <= ((x^2 + 3) (1.5 x^2 + 9.5) + 1) eps <= 7103 eps    (x < 8).
// x >= 8: Mills' ratio by its continued fraction as in mes_math.h (D_k = 1 + k u / D_{k+1}, u = 1 / x^2, depth 16, truncation below
// 1e-16 relative at x = 8): 1 - x R = (u / D_2) / D_1 = u P_3 / P_1, a quotient of positive quantities, no difference: <= 64 eps with
// the exponential (exp(-x^2 / 4) squared, as mes_g, so that only the last product rounds into the subnormals).  x >= 39: +0.
//     KG_H_REL = 7200 eps covers both pieces.
//
// ERROR BOUND of the value, against the exact KG of the doubles consumed (the tests assert THIS, tests/kg_ref.py: kg_bound).
// Let d_j = |b_j - b_0|, S = max_j d_j (at most the spread of the slopes), and T = sum_{j on} d_j (H(lo_j) + H(hi_j)) over the
// exact envelope.
//   relative part: a crossing is one subtraction of the intercepts, one of the slopes (each exact to eps: the inputs are the doubles)
//     and a division: 3 eps relative, which moves H by |c| Phi(-|c|) 3 eps <= 0.51 eps -- charged to the absolute part; H itself carries
//     KG_H_REL, the factor (b_j - b_0), the difference of the two H and the product 3 eps, and the n-term sum (n + 1) eps of T:
//         (KG_H_REL + (n + 4) eps) T.
//   absolute part: 2 x 0.51 eps per line from the crossings' rounding, and for NEARLY CONCURRENT lines -- where device and truth may
//     hold different but equally valid envelopes, a line on in one and off in the other -- the width of such an interval is at most
//     the crossings' rounding, 6 eps |c|, and its term at most d_j Phi(-|c|) 6 eps |c| <= 1.02 eps d_j; the intercepts enter only
//     through the crossings (3 eps relative whatever their spread), so the part is proportional to eps times the spread of the SLOPES:
//         2.04 eps n S.
//   flush: every product below 2^-1022 may lose its last bits: n 2^-1022.
//     |KG_computed - KG| <= (KG_H_REL + (n + 4) eps) T + 2.04 eps n S + n 2^-1022        (kg_bound).
// T <= 0.8 n S always, so the bound is below 128 x 0.8 x 8e-13 S ~ 8.2e-11 S: four orders under the 1e-6 parity tolerance it feeds.
// The clamp max(KG, 0) only moves the computed value towards the truth (KG >= 0).
#ifndef GPX_KG_MATH_H
#define GPX_KG_MATH_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPX_KG_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define GPX_KG_FN inline
#endif

namespace gpx {

constexpr int KG_MAX_M = 127;                  // support points
constexpr int KG_MAX_LINES = KG_MAX_M + 1;     // + the candidate's own line, line 0
constexpr int KG_WAYS = 4;                     // interleaved partial sums
constexpr double KG_EPS = 0x1.0p-53;
constexpr double KG_H_REL = 7200.0 * KG_EPS;
constexpr double KG_INV_SQRT2 = 0.70710678118654752440;
constexpr double KG_INV_SQRT_2PI = 0.39894228040143267794;
constexpr double KG_FAR = 8.0;                 // |c| from here on: the continued fraction
constexpr int KG_CF_K = 16;
constexpr double KG_ZERO = 39.0;               // from here on h(-|c|) < 2^-1075: +0
constexpr double KG_INF = __builtin_huge_val();

// H(c) = h(-|c|) = phi(|c|) - |c| (1 - Phi(|c|)): > 0, decreasing in |c|, H(0) = 1 / sqrt(2 pi), H(+-inf) = +0
GPX_KG_FN double kg_H(double c) {
    const double x = fabs(c);
    if (!(x < KG_ZERO)) return 0.0;
    const double h2 = x * x;
    const double l = fma(x, x, -h2);
    if (x >= KG_FAR) {
        const double t = 1.0 / x, u = t * t;
        double b = 1.0, a = fma((double)KG_CF_K, u, 1.0);        // P_{K+1}, P_K
        for (int k = KG_CF_K - 1; k >= 2; --k) {
            const double p = fma((double)k * u, b, a);
            b = a;
            a = p;
        }
        const double p1 = fma(u, b, a);                            // b = P_3, a = P_2
        const double e2 = exp(-0.25 * h2);
        double v = KG_INV_SQRT_2PI * (u * (b / p1));
        v = fma(-0.5 * l, v, v);
        return (v * e2) * e2;
    }
    const double e = exp(-0.5 * h2);
    const double phi = KG_INV_SQRT_2PI * fma(-0.5 * l, e, e);
    const double Q = 0.5 * erfc(x * KG_INV_SQRT2);
    return phi - x * Q;
}

// phi and Phi at a crossing (+-inf: 0 and 0 / 1): the weights of the gradient
GPX_KG_FN double kg_phi(double c) { return KG_INV_SQRT_2PI * exp(-0.5 * c * c); }
GPX_KG_FN double kg_Phi(double c) { return 0.5 * erfc(-c * KG_INV_SQRT2); }

// The interval (lo, hi) on which line j of n is the upper envelope; false: the line is off (hidden by an equal slope, or hi <= lo).
template <class L>
GPX_KG_FN bool kg_interval(int j, int n, const L& ln, double& lo, double& hi) {
    const double aj = ln.a(j), bj = ln.b(j);
    bool on = true;
    lo = -KG_INF;
    hi = KG_INF;
    for (int i = 0; i < n; ++i) {
        const double ai = ln.a(i), bi = ln.b(i);
        if (bi == bj) {
            if (i != j && (ai > aj || (ai == aj && i < j))) on = false;
        } else {
            const double c = (ai - aj) / (bj - bi);
            if (bi < bj) lo = fmax(lo, c);
            else hi = fmin(hi, c);
        }
    }
    return on && hi > lo;
}

// the term of line j: (b_j - bref) (H(lo_j) - H(hi_j)), 0 for a line that is off
template <class L>
GPX_KG_FN double kg_term(int j, int n, const L& ln, double bref) {
    double lo, hi;
    if (!kg_interval(j, n, ln, lo, hi)) return 0.0;
    return (ln.b(j) - bref) * (kg_H(lo) - kg_H(hi));
}

// partial sum t of KG_WAYS: lines t, t + KG_WAYS, .. in ascending order
template <class L>
GPX_KG_FN double kg_partial(int t, int n, const L& ln, double bref) {
    double s = 0.0;
    for (int j = t; j < n; j += KG_WAYS) s += kg_term(j, n, ln, bref);
    return s;
}

GPX_KG_FN double kg_combine(const double (&p)[KG_WAYS]) { return fmax(((p[0] + p[1]) + p[2]) + p[3], 0.0); }

// the whole value in one thread (the host; the device spreads the partial sums over KG_WAYS threads and combines the same way)
template <class L>
GPX_KG_FN double kg_value(int n, const L& ln) {
    double p[KG_WAYS];
    for (int t = 0; t < KG_WAYS; ++t) p[t] = kg_partial(t, n, ln, ln.b(0));
    return kg_combine(p);
}

// What the gradient needs of line j: P_j = Phi(hi_j) - Phi(lo_j), the probability that the line is the maximum, and
// w_j = phi(lo_j) - phi(hi_j), so that dKG = sum_j P_j da_j + sum_j w_j db_j - d(max_j a_j).  Both 0 for a line that is off.
template <class L>
GPX_KG_FN void kg_weights(int j, int n, const L& ln, double& P, double& w) {
    double lo, hi;
    P = 0.0;
    w = 0.0;
    if (!kg_interval(j, n, ln, lo, hi)) return;
    P = kg_Phi(hi) - kg_Phi(lo);
    w = kg_phi(lo) - kg_phi(hi);
}

// lines in two plain arrays (the host checker, the gradient kernel)
struct KgArrays {
    const double *al, *be;
    GPX_KG_FN double a(int i) const { return al[i]; }
    GPX_KG_FN double b(int i) const { return be[i]; }
};

}  // namespace gpx
#endif
