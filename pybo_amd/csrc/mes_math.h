// mes_math.h -- max-value entropy search (Wang & Jegelka 2017): the per-sample term
//     g(c) = c phi(c) / (2 Phi(c)) - log Phi(c),        c = (y* - mu) / sqrt(s2),
// and the kernel-argument block that carries the sampled maxima y*_1 .. y*_S to k_acq_mes (kernels_mes.hip) by value.
#pragma once
#include <hip/hip_runtime.h>

namespace gpx {

constexpr int MES_MAX_S = 64;
// by value in the kernel arguments: asynchronous-safe (nothing to keep alive behind a _dev entry), wave-uniform, read-only
struct MesArg {
    int S;
    double y[MES_MAX_S];
};

constexpr double MES_HALF_LOG_2PI = 0.91893853320467274178;     // log(2 pi) / 2
constexpr double MES_SQRT_HALF_PI = 1.25331413731550025121;     // sqrt(pi / 2)
constexpr double MES_INV_SQRT2 = 0.70710678118654752440;
constexpr double MES_INV_SQRT_2PI = 0.39894228040143267794;
constexpr double MES_FAR = 8.0;        // |c| from here on: Mills' ratio by its continued fraction
constexpr int MES_CF_K = 16;           // its depth (truncation at |c| = 8: 2.3e-17 of g, smaller beyond; tests/test_mes_cpu.py)
constexpr double MES_ZERO = 39.0;      // from here on g(c) < 2^-1075: +0

// Mills' ratio R(x) = (1 - Phi(x)) / phi(x), x >= 8, by its continued fraction R = 1 / (x + 1 / (x + 2 / (x + 3 / ...))).  Scaled by
// t = 1 / x, u = t^2:  x + k / (x D_{k+1}) = x D_k with D_k = 1 + k u / D_{k+1}, R = t / D_1.  D_k = P_k / P_{k+1} by the backward
// recurrence P_k = P_{k+1} + k u P_{k+2} from P_{K+1} = P_{K+2} = 1: FMAs of positive terms, u <= 1 / 64, nothing overflows (the P stay
// below (1 + K / 64)^K) and nothing cancels; at x = +inf every P is 1.  Returns P_1, P_2, P_3.
__device__ __forceinline__ void mes_cf(double u, double& p1, double& p2, double& p3) {
    double b = 1.0, a = fma((double)MES_CF_K, u, 1.0);        // P_{K+1}, P_K
#pragma unroll
    for (int k = MES_CF_K - 1; k >= 2; --k) {
        const double p = fma((double)k * u, b, a);
        b = a;
        a = p;
    }
    p3 = b;
    p2 = a;
    p1 = fma(u, b, a);
}

// g in four pieces; g > 0 everywhere, NaN in -> NaN out, g(+inf) = +0, g(-inf) = +inf, -0 never comes out.
//   0 <= c < 8: both terms are >= 0, no cancellation.  phi = exp(-c^2 / 2) with the rounding of c^2 put back (l = c^2 - fl(c^2) by one
//     FMA, exp(-(h + l) / 2) = exp(-h / 2) (1 - l / 2)).  -log Phi = -log1p(-Q), Q = erfc(c / sqrt 2) / 2 <= 1 / 2.
//   8 <= c < 39: Phi = 1 and -log Phi = Q to 3 eps (Q(8) = 6.2e-16), so g = phi (c / 2 + R(c)), R by the continued fraction -- one
//     product, no erfc whose last bits the subnormals would show.  exp(-h / 2) = exp(-h / 4)^2 with exp(-h / 4) >= 1e-165 normal: the
//     LAST multiplication is the only operation that can round into the subnormals, so the result is within half a spacing there,
//     and it reaches exactly +0 (c = 38.6); from 39 on +0 is returned outright (inf * 0 never forms).
//   -8 <= c < 0: w = Phi / phi = sqrt(pi / 2) erfcx(-c / sqrt 2) (Mills' ratio at -c), and with log Phi = log w - c^2 / 2 - log(2 pi) / 2
//         g = (c / 2) (1 + c w) / w + log(2 pi) / 2 - log w:
//     the two c^2 / 2 of the naive form are gone analytically.  1 + c w still cancels -- it is ~ 1 / c^2 -- and w's relative error e
//     comes out as c^2 e / 2 absolute: at most 32 e here, against g >= log 2.
//   c < -8: x = -c, w = R(x) = t / D_1 and 1 + c w = (u / D_2) / D_1: a quotient of POSITIVE quantities, never a difference, so
//         g = log(2 pi) / 2 - 1 / (2 D_2) + log(x + t / D_2)
//     -- about log x + 0.42 -- holds its relative accuracy for every x; at x = +inf t = u = 0, D = 1, g = log(inf) = +inf.
__device__ __forceinline__ double mes_g(double c) {
    if (c >= MES_ZERO) return 0.0;
    if (c >= MES_FAR) {
        const double h = c * c;
        const double l = fma(c, c, -h);
        const double e2 = exp(-0.25 * h);
        const double t = 1.0 / c;
        double p1, p2, p3;
        mes_cf(t * t, p1, p2, p3);
        double a = MES_INV_SQRT_2PI * fma(t, p2 / p1, 0.5 * c);
        a = fma(-0.5 * l, a, a);
        return (a * e2) * e2;
    }
    if (c >= 0.0) {
        const double h = c * c;
        const double l = fma(c, c, -h);
        const double e = exp(-0.5 * h);
        const double phi = MES_INV_SQRT_2PI * fma(-0.5 * l, e, e);
        const double Q = 0.5 * erfc(c * MES_INV_SQRT2);
        return (0.5 * c) * phi / (1.0 - Q) - log1p(-Q);
    }
    if (c >= -MES_FAR) {
        const double w = MES_SQRT_HALF_PI * erfcx(-c * MES_INV_SQRT2);
        return (0.5 * c) * (1.0 + c * w) / w + (MES_HALF_LOG_2PI - log(w));
    }
    // (NaN arrives here: every comparison above is false, and it propagates)
    const double x = -c;
    const double t = 1.0 / x;
    double p1, p2, p3;
    mes_cf(t * t, p1, p2, p3);
    const double inv_d2 = p3 / p2;
    return (MES_HALF_LOG_2PI - 0.5 * inv_d2) + log(fma(t, inv_d2, x));
}

}  // namespace gpx
