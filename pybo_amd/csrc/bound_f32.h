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
