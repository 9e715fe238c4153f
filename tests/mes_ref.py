"""High-precision truth and a derived error bound for max-value entropy search (pybo_amd/csrc/mes_math.h mes_g, kernels_mes.hip
k_acq_mes), in the mould of tests/devmath_ref.py.

    gamma_s = (y*_s - mu) / sqrt(s2)        g(c) = c phi(c) / (2 Phi(c)) - log Phi(c)        MES = (1 / S) sum_s g(gamma_s)

The truth is evaluated with mpmath AT THE DOUBLES THE DEVICE CONSUMED (mu, s2, y*), so the bound measures the device's arithmetic
alone.  eps = 2^-52, u = eps / 2, TINY = 2^-1074.  `mes_value` (pybo_amd/mes.py) is the numpy closure of the whole policy value on
(mu, s2): the device's pieces operation for operation, without its FMAs.
"""
import mpmath as mp
import numpy as np

from pybo_amd.mes import mes_value            # noqa: F401  (the numpy closure: re-exported for the tests)

mp.mp.dps = 50

EPS = 2.0 ** -52
U = 2.0 ** -53
TINY = 2.0 ** -1074
FAR = 8.0                   # csrc/mes_math.h: MES_FAR, MES_CF_K, MES_ZERO
CF_K = 16
ZERO = 39.0
# budgets for the device library's functions, relative: exp, log and log1p are documented within 1 - 2 ulp, erfc and erfcx within a
# few (OpenCL's own limit for erfc is 16 ulp; none is hand-written here, so none can be derived)
E_EXP = 2 * EPS
E_LOG = 2 * EPS
E_ERF = 8 * EPS
E_CF = (2 * CF_K + 8) * U   # p3 / p2, p2 / p1 of the continued fraction: K FMAs of positive terms in u (itself 2.5 u), one division
ASYM = -1.0e8               # below: the truth by the asymptotic series (the closed form would need > 100 digits)


def _mp(x):
    return mp.mpf(float(x))


def _digits(c):
    """Working digits for the closed form at c: both of its terms are ~ c^2 / 2 for c << 0 and cancel to ~ log|c|."""
    return 60 + (int(4 * mp.log10(abs(c))) if abs(c) > 10 else 0)


def _tail(c):
    """(x, 1 - x R(x), x R(x)) for x = -c >= 1e8 by the asymptotic series 1 - x R = 1/x^2 - 3/x^4 + 15/x^6 - 105/x^8 (next term < 1e-77)."""
    x = -c
    v = 1 / (x * x)
    one_minus = v * (1 - v * (3 - v * (15 - 105 * v)))
    return x, one_minus, 1 - one_minus


def g_truth(c):
    """g at the mpf c (NaN -> NaN, +inf -> 0, -inf -> +inf)."""
    if mp.isnan(c):
        return mp.nan
    if c == mp.inf:
        return mp.mpf(0)
    if c == -mp.inf:
        return mp.inf
    if c > -ASYM:
        return mp.mpf(0)                       # (below 2^-(10^15): 0 for every purpose here)
    if c < ASYM:
        x, om, xr = _tail(c)                   # w = R = xr / x:  g = -(x / 2) om / R + log(2 pi) / 2 - log R
        return -(x * x / 2) * om / xr + mp.log(2 * mp.pi) / 2 - mp.log(xr / x)
    with mp.workdps(_digits(c)):
        if c >= 0:
            q = mp.ncdf(-c)
            return +(c * mp.npdf(c) / (2 * (1 - q)) - mp.log1p(-q))
        p = mp.ncdf(c)
        return +(c * mp.npdf(c) / (2 * p) - mp.log(p))


def dg_truth(c):
    """g'(c) = -(h / 2) (1 + c^2 + c h), h = phi / Phi (finite c); far left g' -> 1 / c."""
    if c < ASYM:
        return 1 / c
    with mp.workdps(_digits(c) + 20):
        h = mp.npdf(c) / mp.ncdf(c)
        return +(-(h / 2) * (1 + c * c + c * h))


def gamma_truth(mu, s2, y):
    return (_mp(y) - _mp(mu)) / mp.sqrt(_mp(s2))


def mes_truth(mu, s2, ystar):
    """MES at the doubles (mu, s2, y*_1..S): an mpf (NaN moment -> NaN)."""
    if np.isnan(mu) or np.isnan(s2):
        return mp.nan
    ystar = np.asarray(ystar, dtype=float).reshape(-1)
    return mp.fsum(g_truth(gamma_truth(mu, s2, y)) for y in ystar) / len(ystar)


def g_bound(c, g=None):
    """Absolute bound for the device's g at the exact gamma c (mpf), derived from mes_g's operations.  Two parts.

    1. gamma.  The device forms it by a difference, a square root and a quotient: |d gamma| <= 3 u |gamma| (to first order; 1.001
       covers the second), which g turns into 3 u |gamma g'(gamma)| -- the condition |gamma g' / g| is at most gamma^2 for gamma > 0
       (g ~ gamma phi / 2) and about 1 / log|gamma| far left (g ~ log|gamma|, g' ~ 1 / gamma).
    2. the piece in use (a gamma within 4 u of a switch-over may take either: the larger bound), with E_* the budgets above:
       0 <= c < 8:   T1 = (c / 2) phi / (1 - Q), T2 = -log1p(-Q), Q = erfc(c / sqrt 2) / 2.  phi = k exp(-h / 2) (1 - l / 2): exp, the
                     constant, two roundings -> E_EXP + 3 u.  Q: the scaled argument carries 1.5 u, erfc's condition is <= 1 + c^2 ->
                     rQ = 1.5 u (1 + c^2) + E_ERF.  1 - Q >= 1 / 2 moves by 2 Q rQ + u; product and quotient 2 u:
                     |dT1| <= T1 (E_EXP + 6 u + 2 Q rQ).  dT2 = dQ / (1 - Q) <= 2 T2 rQ (T2 >= Q), plus log1p: |dT2| <= T2 (2 rQ + E_LOG).
                     The difference: u g.
       8 <= c < 39:  g = ((k (c / 2 + R) (1 - l / 2)) e2) e2, e2 = exp(-h / 4), R = t p2 / p1.  Dropping Phi = 1 - Q and log1p's second
                     order: <= Q(8) = 6.2e-16 < 3 eps.  R is at most 1 / 32 of the bracket: (E_CF + 2 u) / 32; the bracket, the
                     constant, the FMA and the two products: 6 u; e2 twice: 2 E_EXP.  Only the last product can round into the
                     subnormals: that half spacing is the TINY of mes_bound.
       -8 <= c < 0:  w = k' erfcx(-c / sqrt 2): rw = 1.5 u (argument; erfcx's condition is <= 1) + E_ERF + 1.5 u.  1 + c w, |c w| <= 1:
                     absolute rw + 2 u -- THE cancellation: divided by w ~ 1 / |c| and multiplied by |c| / 2 it is (|c| / (2 w)) (rw + 2 u),
                     about c^2 rw / 2.  A = (c / 2)(1 + c w) / w also carries |A| (rw + 3 u).  B = log(2 pi) / 2 - log w: rw + E_LOG |log w|
                     + 1.5 u |B|.  The sum: u g.
       c < -8:       g = (H - p3 / (2 p2)) + log(x + t p3 / p2): the first bracket E_CF / 2 + 1.5 u absolute; the logarithm's argument moves
                     by (E_CF + u) / 64 + u relative (t p3 / p2 <= x / 64), which is the logarithm's absolute error, plus E_LOG |log|; the
                     sum: u g.
       Both continued-fraction pieces: the truncation at depth 16, at most u g / 4 (tests/test_mes_cpu.py measures it at |c| = 8).
    """
    if g is None:
        g = g_truth(c)
    if not mp.isfinite(c) or not mp.isfinite(g) or c > -ASYM:
        return 0.0
    part1 = 1.001 * 3 * U * abs(c * dg_truth(c))
    near = lambda edge: abs(c - edge) <= 4 * U * abs(edge) + (TINY if edge == 0 else 0)      # noqa: E731
    pieces = []
    if (0 <= c < FAR) or near(0) or near(FAR):
        cc = max(c, mp.mpf(0))
        q = mp.ncdf(-cc)
        t1 = cc * mp.npdf(cc) / (2 * (1 - q))
        t2 = -mp.log1p(-q)
        rq = 1.5 * U * (1 + cc * cc) + E_ERF
        pieces.append(t1 * (E_EXP + 6 * U + 2 * q * rq) + t2 * (2 * rq + E_LOG) + U * g)
    if (FAR <= c) or near(FAR):
        pieces.append(g * (3 * EPS + (E_CF + 2 * U) / 32 + 6 * U + 2 * E_EXP + U / 4))
    if (-FAR <= c < 0) or near(0) or near(-FAR):
        cc = min(c, -mp.mpf(TINY))
        w = mp.ncdf(cc) / mp.npdf(cc)
        rw = 3 * U + E_ERF
        a = abs(cc / 2 * (1 + cc * w) / w)
        b = mp.log(2 * mp.pi) / 2 - mp.log(w)
        pieces.append(abs(cc) / (2 * w) * (rw + 2 * U) + a * (rw + 3 * U) + rw + E_LOG * abs(mp.log(w)) + 1.5 * U * abs(b) + U * g)
    if (c < -FAR) or near(-FAR):
        x = -c
        pieces.append(E_CF / 2 + 1.5 * U + (E_CF + U) / 64 + U + E_LOG * abs(mp.log(x)) + U * g + U * g / 4)
    return float(part1 + max(pieces))


def mes_bound(mu, s2, ystar, t=None):
    """Absolute bound for the device's MES value at the doubles (mu, s2, y*_1..S) (t: the truth, if the caller has it).
    Each g_s within g_bound; the S-term sum in s ascending adds gamma_{S-1} = (S - 1) u / (1 - (S - 1) u) of the (positive) sum, the
    one division u; one smallest-subnormal spacing TINY absolute (the far-right piece's last product, a subnormal quotient)."""
    ystar = np.asarray(ystar, dtype=float).reshape(-1)
    S = len(ystar)
    cs = [gamma_truth(mu, s2, y) for y in ystar]
    gs = [g_truth(c) for c in cs]
    if t is None:
        t = mp.fsum(gs) / S
    if not mp.isfinite(t):
        return 0.0
    gam = (S - 1) * U / (1 - (S - 1) * U)
    return float(mp.fsum(g_bound(c, g) for c, g in zip(cs, gs)) / S + (gam + U) * t * (1 + gam)) + TINY


def check_mes(mu, s2, ystar, got):
    """(violations, worst ratio) of the values `got` (M,) at the moments (mu, s2) (M,) for the maxima ystar: (S,) shared or (M, S) per
    candidate.  NaN moments must give NaN, an infinite truth must be matched exactly."""
    mu, s2, got = (np.asarray(a, dtype=float) for a in (mu, s2, got))
    ystar = np.asarray(ystar, dtype=float)
    bad = np.zeros(len(mu), dtype=bool)
    worst = 0.0
    for i in range(len(mu)):
        ys = ystar[i] if ystar.ndim == 2 else ystar
        t = mes_truth(mu[i], s2[i], ys)
        if mp.isnan(t):
            bad[i] = not np.isnan(got[i])
            continue
        if not mp.isfinite(t):
            bad[i] = got[i] != float(t)
            continue
        if not np.isfinite(got[i]):
            bad[i] = True
            continue
        ratio = float(abs(_mp(got[i]) - t)) / mes_bound(mu[i], s2[i], ys, t)
        bad[i] = ratio > 1.0
        worst = max(worst, ratio)
    return bad, worst


def naive_g(c):
    """The two-term form as written, in doubles: what the bound must NOT bless."""
    from scipy.special import ndtr
    c = np.asarray(c, dtype=float)
    with np.errstate(all='ignore'):
        cdf = ndtr(c)
        return c * (0.39894228040143267794 * np.exp(-0.5 * c * c)) / (2.0 * cdf) - np.log(cdf)


def naive_g_log(c):
    """The naive form at its best: each term as accurate as a double allows (log Phi from log_ndtr), then subtracted."""
    from scipy.special import log_ndtr
    c = np.asarray(c, dtype=float)
    with np.errstate(all='ignore'):
        lp = log_ndtr(c)
        return 0.5 * c * np.exp(-0.5 * c * c - 0.91893853320467274178 - lp) - lp
