// gpx_math.h -- the covariance functions, shared by every kernel that evaluates one (Gram build, cross-Gram,
// gradient path) so that K, K* and dK*/dx come from the same arithmetic.
// Also the acquisition value from the posterior moments (acq_value): the sweep's k_acq and the batch scoring of kernels_batch.hip share it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gpx.h"

namespace gpx {

// exp(x) for x <= 0 -- the only arguments a stationary covariance produces.  Cody-Waite reduction
// x = k ln2 + r (|r| <= ln2/2; ln2 split so that k*ln2_hi is exact), Taylor polynomial of degree 13 in Horner
// form (remainder r^14/14! < 4e-18 relative), scaling by v_ldexp_f64 (which also produces the denormal /
// zero tail); NaN propagates.  Measured against a 50-digit reference: <= 0.79 ulp, the same as the library's.
// Why not the library exp: the cross-Gram is VALU-issue-bound (PMC: SQ_INSTS_VALU x 4 cycles = its run time,
// 73 instructions per K* entry) and two thirds of the library call's instruction slots were v_mov_b32 pairs
// re-materialising its 64-bit literals in VGPRs for every evaluation.  The coefficients here live in
// constant memory, so they arrive by scalar loads and feed v_fma_f64 directly as its one SGPR operand.
__constant__ double kExpC[16] = {
    1.60590438368216133e-10, 2.08767569878681002e-09, 2.50521083854417202e-08, 2.75573192239858883e-07,
    2.75573192239858925e-06, 2.48015873015873016e-05, 1.98412698412698413e-04, 1.38888888888888894e-03,
    8.33333333333333322e-03, 4.16666666666666644e-02, 1.66666666666666657e-01, 0.5,
    1.44269504088896340736,           // [12] 1/ln2
    -6.93147180369123816490e-01,      // [13] -ln2_hi (21 trailing zero bits)
    -1.90821492927058770002e-10,      // [14] -ln2_lo
    -746.0};                          // [15] below this exp() is 0 in fp64
// 1.5 * 2^52: fma(x, 1/ln2, kExpMagic) is that constant plus the integer nearest x / ln2 (one rounding), the integer
// itself sits in the low mantissa bits -- the low dword IS k in two's complement for |k| < 2^31 -- and subtracting the
// constant again returns it as a double: v_rndne_f64 and v_cvt_i32_f64 (0.7 of an FMA's issue rate) are not needed.
__constant__ double kExpMagic = 6755399441055744.0;

__device__ __forceinline__ double exp_nonpos(double x) {
    x = (x < kExpC[15]) ? kExpC[15] : x;                        // NaN passes through
    const double t = fma(x, kExpC[12], kExpMagic);
    const double k = t - kExpMagic;
    double r = fma(k, kExpC[13], x);
    r = fma(k, kExpC[14], r);
    double p = kExpC[0];
#pragma unroll
    for (int i = 1; i < 12; ++i) p = fma(p, r, kExpC[i]);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, __double2loint(t));                         // (t NaN: p is NaN too)
}

// sqrt of a squared distance: x >= 0 (a sum of squares) or NaN.  v_rsq_f64 seed (5e-8) + one coupled Goldschmidt step +
// two residual corrections -- the library's own iteration without its range scaling (4 instructions shorter): arguments
// below 1e-280 (distances below 1e-140 length scales) give 0, which is what their covariance rounds to anyway.
// x >= 1e300, +inf included (an overflowed scaled distance: very small length scales), gives `top` instead: every
// covariance is 0 there, and `top` is chosen by the caller so that it stays 0 and not NaN (rsq(inf) = 0 would make g
// NaN): Matern-1/2 passes x itself (exp(-x) = 0, also for +inf), Matern-5/2 and -3/2 pass 512, whose exponentials
// exp(-sqrt(5) 512) and exp(-sqrt(3) 512) underflow to 0 as well while their polynomial factors stay finite (an
// overflowed polynomial times 0 is NaN).  512 is an inline constant of the select (no register, no instruction).
__device__ __forceinline__ double sqrt_r2(double x, double top) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    double e = fma(-g, g, x);
    g = fma(e, h, g);
    e = fma(-g, g, x);
    g = fma(e, h, g);
    return (x > 1.0e-280) ? ((x < 1.0e300) ? g : top) : x * 0.0;    // 0 -> 0, NaN -> NaN
}

// the polynomial factors of the Matern covariances in s = sqrt(2 nu) r.  Matern-5/2's 1 + s + 5/3 r^2 is written in s alone
// (s^2 / 3 = 5/3 r^2), which stays finite for every s sqrt_r2 leads to -- (5/3) r2 overflows from r2 = 1.08e308 on; two
// FMAs, as many as 1 + s + (5/3) r2 took
__device__ __forceinline__ double m52_poly(double s) { return fma(s, fma(s, 1.0 / 3.0, 1.0), 1.0); }
__device__ __forceinline__ double m32_poly(double s) { return 1.0 + s; }

// covariance as a function of the squared scaled distance r2 = sum_k ((x_k - z_k)/ell_k)^2.  kern_and_grad
// (kernels_grad.hip) evaluates its k by the same expressions in the same order: every path returns the same bits
// for the same r2 (tests/test_gpu_devmath.py).  Accuracy there, against a 50-digit reference at the r2 consumed:
// SE <= 1 ulp (normal results), Matern <= (3 + 2 s) eps relative; 0 wherever the exponential underflows, +inf included.
__device__ __forceinline__ double kern_eval(int kid, double r2, double rho) {
    switch (kid) {
        case GPX_KERN_SE_ARD:
            return rho * exp_nonpos(-0.5 * r2);
        case GPX_KERN_MATERN52: {
            const double s = 2.23606797749978969641 * sqrt_r2(r2, 512.0);
            return rho * m52_poly(s) * exp_nonpos(-s);
        }
        case GPX_KERN_MATERN32: {
            const double s = 1.73205080756887729353 * sqrt_r2(r2, 512.0);
            return rho * m32_poly(s) * exp_nonpos(-s);
        }
        default:
            return rho * exp_nonpos(-sqrt_r2(r2, r2));
    }
}

// k and g = dk/dr2 (the input gradients of kernels_grad.hip, the evidence gradient of kernels_hyper.hip); k is kern_eval's
// expression, operation for operation (rho * poly * exp, associated from the left), so that K* here and in the cross-Gram /
// Gram are the same bits
__device__ __forceinline__ void kern_and_grad(int kid, double r2, double rho, double& k, double& g) {
    switch (kid) {
        case GPX_KERN_SE_ARD: {
            k = rho * exp_nonpos(-0.5 * r2);
            g = -0.5 * k;
            break;
        }
        case GPX_KERN_MATERN52: {
            const double s = 2.23606797749978969641 * sqrt_r2(r2, 512.0);
            const double x = exp_nonpos(-s);
            k = rho * m52_poly(s) * x;
            g = -(5.0 / 6.0) * (1.0 + s) * (rho * x);
            break;
        }
        case GPX_KERN_MATERN32: {
            const double s = 1.73205080756887729353 * sqrt_r2(r2, 512.0);
            const double x = exp_nonpos(-s);
            k = rho * m32_poly(s) * x;
            g = -1.5 * (rho * x);
            break;
        }
        default: {
            const double r = sqrt_r2(r2, r2);
            k = rho * exp_nonpos(-r);
            // exp(-r) has a kink at r = 0 (a candidate on top of an observation: the L-BFGS seeds of the
            // recommender ARE observations): dk/dx is +-k/ell from either side, take the symmetric value 0.  The same 0 for
            // every r2 <= 1e-280 (distances below 1e-140 length scales), where sqrt_r2 returns 0: such a candidate is
            // treated as sitting on the observation (tests/test_gpu_devmath.py pins both sides of that cutoff)
            g = (r > 0.0) ? -0.5 * k / r : 0.0;
        }
    }
}

// ---- acquisition values ----------------------------------------------------------------------------------------
__device__ __forceinline__ double norm_cdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }
__device__ __forceinline__ double norm_pdf(double z) {
    return 0.39894228040143267794 * exp(-0.5 * z * z);
}

// The acquisition value from the posterior moments: the ONE place this arithmetic lives.  k_acq calls it with a candidate's
// exact moments (acq_core.h: cand_moments), the bound passes of a selection-only sweep through ei_mean_bound below.
__device__ __forceinline__ double acq_value(int acq_id, double mu, double s2, double p0) {
    switch (acq_id) {
        case GPX_ACQ_EI: {
            const double s = sqrt(s2);
            const double dlt = mu - p0;
            const double z = dlt / s;
            return dlt * norm_cdf(z) + s * norm_pdf(z);
        }
        case GPX_ACQ_PI: {
            const double z = (mu - p0) / sqrt(s2);
            return norm_cdf(z);
        }
        case GPX_ACQ_UCB:
            return mu + sqrt(p0 * s2);
        default:
            return mu;
    }
}

// The EI mean bound of the pruned sweeps (k_prune_ub, k_prune_ub2, k_prune_ub_fold): EI by k_acq's own function at an upper bound of
// the mean -- dot = alpha2 . k(X, z), delta = the bound pass's margin, added in this order -- and a variance s2 no smaller than the exact one.
__device__ __forceinline__ double ei_mean_bound(double bias, double dot, double delta, double s2, double p0) {
    return acq_value(GPX_ACQ_EI, (bias + dot) + delta, s2, p0);
}

// (the bound pass's matrix-pipe kernels, kernels_sweep.hip and kernels_bound32.hip)
// z~ of one candidate coordinate: the cross-Gram's own scaled value, then the centring -- two roundings, never one fused
__device__ __forceinline__ double bound_zt(double z, double invell, double c) {
#pragma clang fp contract(off)
    const double zs = z * invell;
    return zs - c;
}

}  // namespace gpx
