"""High-precision truth and error bounds for the device math of pybo_amd/csrc (gpx_math.h: exp_nonpos, sqrt_r2, kern_eval;
kernels_grad.hip: kern_and_grad; kernels_rff.hip: cos_cw; kernels_sweep.hip: the EI / PI / UCB lines of k_acq).

Every truth is evaluated with mpmath at 50 digits AT THE DOUBLE THE DEVICE CONSUMED (the r2, z or (mu, s2, p0) it was
given), so a bound measures the primitive alone.  Every checker returns a boolean mask of the entries that violate its
bound (True = violation) and the worst ratio error / bound, so a test can report both.  The bounds are derived in the
docstrings; eps = 2^-52 (one ulp of 1), u = eps / 2 (the unit roundoff).
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50

EPS = 2.0 ** -52
U = 2.0 ** -53
TINY = 2.0 ** -1074                     # the smallest subnormal: the spacing of the whole subnormal band
KIDS = {'se': 0, 'matern5': 1, 'matern3': 2, 'matern1': 3}

# the two doubles of cos_cw's Cody-Waite split of pi (kernels_rff.hip) and the third term it drops, exactly
PI_HI = 3.14159265346825122833e+00
PI_LO = 1.21542010126079319532e-10
C3 = abs(float(mp.pi - mp.mpf(PI_HI) - mp.mpf(PI_LO)))      # 4.04e-21
INV_PI = 3.18309886183790671538e-01
COS_POLY_ABS = 3e-16                                          # cos_cw's error on the reduced argument (derivation below)


def _mp(x):
    return mp.mpf(float(x))


# ---------------------------------------------------------------------------------------------------------------------
# truth
# ---------------------------------------------------------------------------------------------------------------------
def _kern_s(kid, r2):
    """(s, poly) of the covariance at the exact r2: k = rho * poly * exp(-s)."""
    if kid == 0:
        return r2 / 2, mp.mpf(1)
    r = mp.sqrt(r2)
    if kid == 1:
        s = mp.sqrt(5) * r
        return s, 1 + s + s * s / 3
    if kid == 2:
        s = mp.sqrt(3) * r
        return s, 1 + s
    return r, mp.mpf(1)


def kern_truth(kid, r2, rho):
    """k(r2) = rho * poly * exp(-s) at 50 digits: an mpf (inf r2 -> 0, NaN r2 -> NaN)."""
    r2 = float(r2)
    if np.isnan(r2):
        return mp.nan
    if np.isinf(r2):
        return mp.mpf(0)
    s, poly = _kern_s(kid, _mp(r2))
    return _mp(rho) * poly * mp.exp(-s)


def dkdr2_truth(kid, r2, rho):
    """g = dk/dr2 at 50 digits (r2 > 0): SE -k/2, M52 -(5/6)(1+s) rho e^-s, M32 -(3/2) rho e^-s, M12 -rho e^-r / (2r)."""
    r2 = _mp(r2)
    rho = _mp(rho)
    if kid == 0:
        return -rho * mp.exp(-r2 / 2) / 2
    r = mp.sqrt(r2)
    if kid == 1:
        s = mp.sqrt(5) * r
        return -mp.mpf(5) / 6 * (1 + s) * rho * mp.exp(-s)
    if kid == 2:
        s = mp.sqrt(3) * r
        return -mp.mpf(3) / 2 * rho * mp.exp(-s)
    return -rho * mp.exp(-r) / (2 * r)


def norm_cdf(z):
    return mp.ncdf(z)


def norm_pdf(z):
    return mp.npdf(z)


def acq_truth(acq, mu, s2, p0):
    """EI / PI / UCB of kernels_sweep.hip k_acq at the device's own (mu, s2, p0) doubles, 50 digits."""
    mu, s2, p0 = _mp(mu), _mp(s2), _mp(p0)
    if acq == 'ucb':
        return mu + mp.sqrt(p0 * s2)
    s = mp.sqrt(s2)
    dlt = mu - p0
    z = dlt / s
    if acq == 'pi':
        return norm_cdf(z)
    return dlt * norm_cdf(z) + s * norm_pdf(z)


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def _spacing(t):
    """ulp of the double nearest to the mpf t (>= TINY)."""
    return max(float(np.spacing(abs(float(t)))), TINY)


def check_cov(kid, r2, got, rho=1.0):
    """Covariance bound.  Returns (violations, worst ratio).

    SE, rho = 1: the value is exp_nonpos(-r2/2) alone (-0.5 r2 is exact): <= 1 ulp of the result for normal results
    (the polynomial's truncation is 4e-18 relative, Horner over 13 FMAs plus the ldexp stays below 0.8 ulp), <= 1 unit of
    2^-1074 in the subnormal band (ldexp rounds once there), exactly 0 past underflow (truth below 2^-1076: 0 is the
    nearest double by a wide margin; between 2^-1076 and 2^-1075 one unit is allowed, as in the band).  rho != 1 adds the
    product's rounding: 1 ulp of exp, scaled by rho, is at most 2 ulp of the product, plus 1/2 ulp -> 2.5 ulp.

    Matern: s = sqrt(2 nu) * sqrt_r2(r2) carries the constant's rounding (u/2 relative), sqrt_r2's (1 ulp = eps) and the
    product's (u): |ds| <= 2 eps s, which exp(-s) turns into 2 s eps relative.  exp_nonpos's own error (<= 1 ulp = eps),
    the polynomial (two FMAs: 2u) and the two products (rho * poly, * exp: 2u) add 3 eps -> (3 + 2 s) eps relative.  Where
    exp(-s) is subnormal its rounding is absolute (<= 1 unit of 2^-1074), multiplied by rho * poly: + (rho poly + 1) 2^-1074.
    Matern-1/2 is the same with poly = 1, sqrt(2 nu) = 1.
    """
    r2 = np.asarray(r2, dtype=float)
    got = np.asarray(got, dtype=float)
    bad = np.zeros(len(r2), dtype=bool)
    worst = 0.0
    for i, (x, g) in enumerate(zip(r2, got)):
        t = kern_truth(kid, x, rho)
        if mp.isnan(t):
            bad[i] = not np.isnan(g)
            continue
        if np.isnan(g) or np.isinf(g):
            bad[i] = True
            continue
        err = abs(_mp(g) - t)
        if kid == 0:
            if t < mp.mpf(2) ** -1076:
                tol = 0.0
            else:
                tol = _spacing(t) * (1.0 if rho == 1.0 else 2.5)
        else:
            if np.isinf(x) or x >= 1e300:
                tol = 0.0                                          # exp(-s) underflowed: exactly 0, never NaN
            else:
                s, poly = _kern_s(kid, _mp(x))
                tol = float((3 + 2 * s) * EPS * t + (_mp(rho) * poly + 1) * TINY)
        if tol == 0.0:
            bad[i] = g != 0.0
            worst = max(worst, np.inf if g != 0.0 else 0.0)
        else:
            ratio = float(err) / tol
            bad[i] = ratio > 1.0
            worst = max(worst, ratio)
    return bad, worst


def check_grad(kid, x, got, rho=1.0):
    """Gradient bound: the device returns dmu/dx = fl(g * 2x) for the probe (one observation at 0, alpha = 1, ell = 1;
    2x is exact).  g = dk/dr2 carries the covariance's error form, (3 + 2 s) eps relative plus the subnormal term
    (SE: -0.5 k, exact scaling of k; M52: (1 + s) and two more products; M32: one more product; M12: the division by r, whose
    own error is 1 ulp of sqrt_r2 -- all inside the 3 eps), and the final product adds u.  Returns (violations, worst)."""
    x = np.asarray(x, dtype=float)
    got = np.asarray(got, dtype=float)
    bad = np.zeros(len(x), dtype=bool)
    worst = 0.0
    for i, (xi, g) in enumerate(zip(x, got)):
        r2 = xi * xi
        if not np.isfinite(g):
            bad[i] = True
            continue
        if np.isinf(r2) or r2 >= 1e300:
            bad[i] = g != 0.0
            continue
        t = 2 * _mp(xi) * dkdr2_truth(kid, r2, rho)
        s, poly = _kern_s(kid, _mp(r2))
        if kid == 0:
            s = mp.mpf(0)                       # exp(-r2/2) has an exact argument: no conditioning term
        tol = float((3 + 2 * s) * EPS * abs(t) + U * abs(t) + abs(2 * _mp(xi)) * (_mp(rho) * (1 + s) + 1) * TINY + TINY)
        ratio = float(abs(_mp(g) - t)) / tol
        bad[i] = ratio > 1.0
        worst = max(worst, ratio)
    return bad, worst


def cos_cw_n(z):
    """n = round(z / pi) as cos_cw computes it (the magic-number FMA; numpy's rint of the rounded quotient is the same
    integer except within 1e-16 relative of a half-integer, where either choice keeps |r| <= pi/2 + 1e-7)."""
    return np.rint(np.asarray(z, dtype=float) * INV_PI)


def check_cos(z, got, library=False):
    """cos bound, absolute.  cos_cw (library=False): r = z - n pi_hi is exact (one FMA: the product is exact inside the
    FMA and the difference is a multiple of 2^-52 below 2 in magnitude, so it is a double), r - n pi_lo rounds once
    (<= u |r| <= 2e-16 * 1/2), the dropped third term of pi is |n| C3; the Taylor series through r^20/20! is truncated at
    1.8e-17 at |r| = pi/2, and Horner over terms summing to cosh(pi/2) = 2.5 rounds to <= 10 u * ... below 1e-16: together
    COS_POLY_ABS = 3e-16, plus |n| C3 for the reduction.  The library cos (library=True): 2 ulp of the result, relative
    (its reduction is exact).  Returns (violations, worst)."""
    z = np.asarray(z, dtype=float)
    got = np.asarray(got, dtype=float)
    bad = np.zeros(len(z), dtype=bool)
    worst = 0.0
    n = cos_cw_n(z)
    for i, (zi, g) in enumerate(zip(z, got)):
        if np.isnan(zi):
            bad[i] = not np.isnan(g)
            continue
        t = mp.cos(_mp(zi))
        if library:
            tol = 2 * _spacing(t)
        else:
            tol = COS_POLY_ABS + abs(float(n[i])) * C3
        ratio = float(abs(_mp(g) - t)) / tol if np.isfinite(g) else np.inf
        bad[i] = ratio > 1.0
        worst = max(worst, ratio)
    return bad, worst


def check_sin(z, got):
    """-sin(z) from the library (rff_eval_grad's gradient): 2 ulp of the result."""
    z = np.asarray(z, dtype=float)
    got = np.asarray(got, dtype=float)
    bad = np.zeros(len(z), dtype=bool)
    worst = 0.0
    for i, (zi, g) in enumerate(zip(z, got)):
        t = -mp.sin(_mp(zi))
        ratio = float(abs(_mp(g) - t)) / (2 * _spacing(t))
        bad[i] = ratio > 1.0
        worst = max(worst, ratio)
    return bad, worst


def acq_bound(acq, mu, s2, p0, t):
    """Absolute bound for one acquisition value (t: the truth).
    z = (mu - p0) / sqrt(s2) carries three roundings (difference, sqrt, quotient): |dz| <= 3 u |z|.
    PI = Phi(z) = erfc(-z / sqrt 2) / 2: the argument's scaling adds one more rounding, and d log Phi / dz -> |z| for
    z << 0, so those four roundings cost 4 u z^2 = 2 z^2 eps; erfc's own <= 2 ulp = 2 eps (+ 2 more of slack) -> (4 + 4 z^2)
    eps relative.  EI = dlt Phi(z) + s phi(z): Phi and phi = exp(-z^2/2)/sqrt(2 pi) each carry ~4 u z^2 from z plus a few
    roundings, and for z << 0 the two terms cancel to s phi / z^2: the absolute error s phi * O(z^2 eps) is O(z^4 eps)
    relative, C (1 + z^2)^2 eps with C = 6.  UCB = mu + sqrt(p0 s2): the product (u), halved by the sqrt, the sqrt (u) and
    the sum (u) -> 3 ulp.  Results in the subnormal band (z < -37.5) carry an absolute rounding of (|dlt| + s + 1) units
    of 2^-1074 from Phi, phi and their products."""
    mu, s2, p0 = float(mu), float(s2), float(p0)
    if acq == 'ucb':
        return 3 * _spacing(t)
    s = np.sqrt(s2)
    z = (mu - p0) / s
    floor = 4 * (abs(mu - p0) + s + 1) * TINY
    if acq == 'pi':
        return float((4 + 4 * z * z) * EPS * abs(t)) + floor
    return float(6 * (1 + z * z) ** 2 * EPS * abs(t)) + floor


def check_acq(acq, mu, s2, p0, got):
    """Returns (violations, worst) of acq values `got` at the device's (mu, s2) and the target p0 (scalar or array)."""
    mu = np.asarray(mu, dtype=float)
    s2 = np.asarray(s2, dtype=float)
    p0 = np.broadcast_to(np.asarray(p0, dtype=float), mu.shape)
    got = np.asarray(got, dtype=float)
    bad = np.zeros(len(mu), dtype=bool)
    worst = 0.0
    for i in range(len(mu)):
        t = acq_truth(acq, mu[i], s2[i], p0[i])
        if not np.isfinite(got[i]):
            bad[i] = True
            continue
        ratio = float(abs(_mp(got[i]) - t)) / acq_bound(acq, mu[i], s2[i], p0[i], t)
        bad[i] = ratio > 1.0
        worst = max(worst, ratio)
    return bad, worst


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulations of the device primitives (exact FMAs through mpmath): the CPU tests use them to show the bounds bite
# ---------------------------------------------------------------------------------------------------------------------
EXP_C = [1.60590438368216133e-10, 2.08767569878681002e-09, 2.50521083854417202e-08, 2.75573192239858883e-07,
         2.75573192239858925e-06, 2.48015873015873016e-05, 1.98412698412698413e-04, 1.38888888888888894e-03,
         8.33333333333333322e-03, 4.16666666666666644e-02, 1.66666666666666657e-01, 0.5]
COS_C = [4.11031762331216485548e-19, -1.56192069685862264622e-16, 4.77947733238738529744e-14,
         -1.14707455977297247139e-11, 2.08767569878680989792e-09, -2.75573192239858906526e-07,
         2.48015873015873015873e-05, -1.38888888888888888889e-03, 4.16666666666666666667e-02, -0.5]


def fma(a, b, c):
    """Correctly rounded a * b + c for doubles (the exact value at 400 bits, rounded once)."""
    with mp.workprec(400):
        return float(mp.mpf(a) * mp.mpf(b) + mp.mpf(c))


def exp_nonpos_emul(x, coeffs=EXP_C):
    """gpx_math.h exp_nonpos, operation for operation (coeffs[0] is the r^13 coefficient)."""
    x = max(float(x), -746.0)
    t = fma(x, 1.44269504088896340736, 6755399441055744.0)
    k = t - 6755399441055744.0
    r = fma(k, -6.93147180369123816490e-01, x)
    r = fma(k, -1.90821492927058770002e-10, r)
    p = coeffs[0]
    for c in coeffs[1:]:
        p = fma(p, r, c)
    p = fma(p, r, 1.0)
    p = fma(p, r, 1.0)
    return float(np.ldexp(p, int(k)))


def cos_cw_emul(z, coeffs=COS_C):
    """kernels_rff.hip cos_cw, operation for operation (coeffs[0] is the 1/20! term)."""
    t = fma(z, INV_PI, 6755399441055744.0)
    n = t - 6755399441055744.0
    r = fma(-n, PI_HI, z)
    r = fma(-n, PI_LO, r)
    r2 = r * r
    p = coeffs[0]
    for c in coeffs[1:]:
        p = fma(r2, p, c)
    cs = fma(r2, p, 1.0)
    return -cs if int(n) & 1 else cs
