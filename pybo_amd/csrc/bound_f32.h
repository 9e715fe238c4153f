// bound_f32.h -- the error margin of the bound pass's fp32 matrix-pipe kernel (kernels_bound32.hip: k_bound_mfma32), shared with
// tests/c/bound_f32_check.cpp, a host-only program that runs the kernel's arithmetic in float (tests/test_bound_f32_host.py).
// Plain C++ without HIP types.  The derivation is DESIGN.md section 2.1 ("the fp32 bound pass"); in short, with u = 2^-24:
//
//   exponent   e = log2(e) (x~.z~ - |x~|^2/2 - |z~|^2/2) from fp32 copies of log2(e) x~, z~ and the two norms (each formed in fp64 -- the
//              product with log2(e) is one fp64 rounding, 2^-53, far inside the d + 5 for d + 4 below -- and rounded once to fp32)
//              and an fp32 sum of d + 2 terms in any order: |e^ - e| <= eps_e = (log2(e) / 2) (d + 5) (R_x + R_z)^2 u;
//   entry      k^ = v_exp_f32(e^) (documented 1 ulp, 2^-23 relative; twice that granted: u_x = 2^-22), w^ = fl32(w), w 0 or normal: w^ k^ = w k (1 + eta_i),
//              |eta_i| <= eta = 2^eps_e (1 + u_x)(1 + u) - 1;
//   sums       A = sum w^ k^ and B = sum |w^| k^ by n fp32 FMAs a lane (n = Np / 16), the lanes' sums added in fp64:
//              |A - sum w k| <= E0 sum |w| k and B >= (1 - E0) sum |w| k with E0 = g (1 + eta) + eta, g = n u / (1 - n u) + 2^-48;
//   result     dot_hi = A + E / (1 - E) B + F >= sum w k, E = E0 (1 + 2^-8), and dot_hi - sum w k <= 2 E sum |w| k + 3 F for E <= 2^-10
//              (the inflation pays for the 1 / (1 - E) and 1 + E factors of the worst case and the upward rounding; F is lost at
//              most once, added once, and rounded);
//   flush      F = 2^-124 (sum |w| + Np): a covariance below 2^-125 may come back as 0 and an FMA result below 2^-126 may be flushed.
//
// Sign-homogeneous row tiles.  The fp32 copies are written in the order [w > 0][16 extra zero rows][w == 0, the padding rows among
// them][w < 0] (bound32_row_dest), Np + 16 rows: the 16-row tiles [0, tpos), tpos = ceil(npos / 16), hold only w >= 0 and the tiles
// [tpos, Np / 16 + 1) only w <= 0, since at least 16 zero rows lie between the signs.  A wave accumulates P = sum w^ k^ over the first
// group and Nn over the second, ONE FMA per entry, and the lanes form A = P + Nn and B = P - Nn in fp64.  The margin is the same:
//   * an FMA whose weight is 0 and whose k^ is finite returns its accumulator exactly, so it is no rounding step of the sum;
//   * the rows with w > 0 fill at most ceil(npos / 16) <= Np / 16 tiles from row 0 on, the rows with w < 0 end at row Np + 16, a tile
//     boundary, and fill at most ceil(nneg / 16) <= Np / 16 tiles; a wave takes every fourth tile, at most Np / 64 of either group
//     (Np / 16 is a multiple of 8), four rows of each per lane: each of P and Nn sees at most Np / 16 rounding FMAs a lane -- depth = Np / 16 holds;
//   * every term of P is >= 0 and every term of Nn <= 0, so |P - sum+ w k| <= E0 sum+ |w| k and P >= (1 - E0) sum+ |w| k, likewise
//     for Nn, and adding the two: |A - sum w k| <= E0 sum |w| k and B = P - Nn >= (1 - E0) sum |w| k, as before;
//   * the fp64 additions of a candidate are now 16 (one more per lane), 16 x 2^-53 < 2^-48, the term already in g.
//   Same E, same F, same inequality dot_hi - sum w k <= 2 E sum |w| k + 3 F.
//
// Factorised exponent (FACT).  exp(x~.z~ - |x~|^2/2 - |z~|^2/2) = 2^(L x~.z~) r_i c_n with L = log2(e), r_i = 2^(-L |x~_i|^2 / 2) and
// c_n = 2^(-L |z~_n|^2 / 2), both <= 1 (bound32_norm_factor, fp64).  The kernel walks w'_i = fl32(w_i r_i) (the product in fp64) and
// k' = v_exp_f32(e'), e' the fp32 sum of the d products fl32(L x~_k) fl32(z~_k) from a zero accumulator, and multiplies the two fp64 sums
// by c_n once per candidate.  Against the budget above:
//   exponent   |e' - L x~.z~| <= (d + 2) u L |x~||z~| <= (d + 2) u L (R_x + R_z)^2 / 4 (two operand roundings and d - 1 additions on
//              partial sums <= L |x~||z~|; AM-GM), half of eps_e or less; the arguments of the two fp64 exponentials err by
//              2^-52 L (R_x^2 + R_z^2) / 2, far inside the other half: eps_e covers the exponent of w' k' c_n;
//   relative   r_i and c_n within 2 ulp of fp64 each, the products w_i r_i and sum x c_n one rounding each: 6 x 2^-53 on every term,
//              with the 16 additions 22 x 2^-53 < 2^-48, the term in g; fl32(w_i r_i) is the (1 + u) the entry already pays for fl32(w);
//   range      with X = L R_x R_z (1 + 2^-10) >= |e'| the guard bound32_fact_ok asks X <= 120 -- k' lies in [2^-120, 2^120], v_exp_f32
//              neither overflows nor flushes -- and X + log2(sum_w) <= 126, sum_w >= sum |w_i| >= sum |w'_i| -- every partial sum is at
//              most sum |w'| k' (1 + E) < 2^127, finite -- and every w' is 0 (only where w is) or a normal fp32 number
//              (bound32_bad_weight_fact, through k_bound_aug's flag).  No k' is flushed, so the only loss is an FMA result below
//              2^-126 flushed to 0: at most Np 2^-126 <= F / 4 per candidate, in the scaled domain, multiplied by c_n <= 1 afterwards;
//              a c_n that is subnormal or 0 in fp64 moves the product by less than 2^-1022, inside F as well.
//   So E, F and the inequality stand unchanged; where the guard fails the unfactorised walk runs (with the sign tiles).
#ifndef GPX_BOUND_F32_H
#define GPX_BOUND_F32_H

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPX_B32_FN __host__ __device__ __forceinline__
#else
#define GPX_B32_FN inline
#endif

namespace gpx {

constexpr double B32_U = 0x1p-24;                      // unit roundoff of fp32
constexpr double B32_UX = 0x1p-22;                     // relative error granted to v_exp_f32: 2 ulp (documented: 1 ulp = 2^-23)
constexpr double B32_LOG2E = 1.44269504088896340736;   // the operands' pre-scale: v_exp_f32 is 2^x
constexpr double B32_E_MAX = 0x1p-10;                  // the guard: the fp32 kernel runs only where E <= this
constexpr double B32_W_MIN = 0x1p-126, B32_W_MAX = 0x1.fffffep+127;      // the normal range of fp32

// 1.0 where w is neither 0 nor a normal fp32 number once rounded (subnormal, overflowing, not finite): the guard refuses
GPX_B32_FN double bound32_bad_weight(double w) {
    const double a = std::fabs(w);
    return (a == 0.0 || (a >= B32_W_MIN && a <= B32_W_MAX)) ? 0.0 : 1.0;
}

// E of the header comment.  gv = (d + 4)(R_x + R_z)^2 as k_bound_guard forms it; depth = the FMAs of one lane's sum (Np / 16).
// +inf where the radii are not finite or the depth is out of fp32's reach.
GPX_B32_FN double bound32_E(int d, double depth, double gv) {
    const double eps_e = 0.5 * B32_LOG2E * (double)(d + 5) * (gv / (double)(d + 4)) * B32_U;
    const double eta = std::exp2(eps_e) * (1.0 + B32_UX) * (1.0 + B32_U) - 1.0;
    const double nu = depth * B32_U;
    if (!(nu < 0.5) || !(eta < 1.0)) return HUGE_VAL;
    const double g = nu / (1.0 - nu) + 0x1p-48;
    return (g * (1.0 + eta) + eta) * (1.0 + 0x1p-8);
}

// the factor of B in the margin: E / (1 - E), +inf where the derivation does not hold (E >= 1/2 or a weight outside fp32's normal range)
GPX_B32_FN double bound32_factor(double E, double bad_weight) { return (E < 0.5 && bad_weight == 0.0) ? E / (1.0 - E) : HUGE_VAL; }

// F of the header comment; sum_w >= sum |w_i| (k_bound_guard: rho S (1 + 2^-20), S of k_prune_delta)
GPX_B32_FN double bound32_flush(double sum_w, double Np) { return 0x1p-124 * (sum_w + Np); }

// ---- the sign-homogeneous row order of the fp32 copies (header comment) ----
constexpr int B32_ZROWS = 16;                          // the extra all-zero tile between the two signs
// row of the fp32 copies for a weight of sign sgn (> 0, 0, < 0; a NaN weight goes with the zeros) that is the rank-th of its sign
GPX_B32_FN long long bound32_row_dest(int sgn, long long rank, long long npos, long long nzero) {
    return sgn > 0 ? rank : (sgn == 0 ? npos + B32_ZROWS + rank : npos + B32_ZROWS + nzero + rank);
}
// tiles [0, tpos) hold only w >= 0, tiles [tpos, Np / 16 + 1) only w <= 0
GPX_B32_FN long long bound32_tpos(long long npos) { return (npos + 15) / 16; }

// ---- the factorised exponent (header comment, FACT) ----
constexpr double B32_FACT_XMAX = 120.0, B32_FACT_SMAX = 126.0;
// r_i and c_n: 2^(-log2(e) n2 / 2) in fp64, n2 the squared norm of the centred, scaled point
GPX_B32_FN double bound32_norm_factor(double n2) { return std::exp2(B32_LOG2E * (-0.5 * n2)); }
// 1.0 where w is not 0 but w' = w r_i is not a normal fp32 number once rounded
GPX_B32_FN double bound32_bad_weight_fact(double w, double wp) {
    const double a = std::fabs(wp);
    return (w == 0.0 || (a >= B32_W_MIN && a <= B32_W_MAX)) ? 0.0 : 1.0;
}
// the range guard: rx2, rz2 the squared radii, sum_w >= sum |w_i|.  1.0 where the factorised walk may run (a NaN anywhere: 0.0)
GPX_B32_FN double bound32_fact_ok(double rx2, double rz2, double sum_w) {
    const double X = B32_LOG2E * std::sqrt(rx2) * std::sqrt(rz2) * (1.0 + 0x1p-10);
    return (X <= B32_FACT_XMAX && X + std::log2(sum_w) <= B32_FACT_SMAX) ? 1.0 : 0.0;
}

// dot_hi from the two sums: A + factor B + F in fp64, rounded upward (three roundings, each within 2^-53 of |A| + m).
// An infinite factor gives +inf whatever finite B is: the candidate survives every cut.  NaN sums stay NaN (the kernel's fp32 norms
// overflowed, which the guards exclude and only the forced kernel can meet); a NaN bound is kept as a survivor as well.
GPX_B32_FN double bound32_hi(double A, double B, double factor, double F) {
    if (!(factor < HUGE_VAL)) return (A != A || B != B) ? A + B : HUGE_VAL;
    const double m = factor * B + F;
    return std::fma(0x1p-50, std::fabs(A) + m, A + m);
}

}      // namespace gpx
#endif
