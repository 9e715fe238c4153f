"""
Max-value entropy search (Wang & Jegelka 2017) on the host: the arithmetic the device runs in csrc/mes_math.h restated in numpy, the
derivative the models' `get_entropy(..., grad=True)` chain through, and the Gumbel sampler of the maxima y*.

    gamma_s = (y*_s - mu) / sqrt(s2)        g(c) = c phi(c) / (2 Phi(c)) - log Phi(c)        MES = mean_s g(gamma_s)

`mes_g` follows the device's pieces operation for operation (without its FMAs): it is the reference of the CPU tests and the
index of models that have no `get_entropy`.
"""
import numpy as np
from scipy.special import erfc, erfcx, log_ndtr

from .utils import rstate

__all__ = ['mes_g', 'mes_dg', 'mes_value', 'mes_value_grad', 'gumbel_quantiles', 'sample_maxima']

HALF_LOG_2PI = 0.91893853320467274178
SQRT_HALF_PI = 1.25331413731550025121
INV_SQRT2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
FAR = 8.0           # csrc/mes_math.h: MES_FAR, MES_CF_K, MES_ZERO
CF_K = 16
ZERO = 39.0
MAX_S = 64


def _split(c):
    """(hi, lo) halves of c with 26 significant bits each (Veltkamp), so that hi * hi, hi * lo, lo * lo are exact."""
    t = 134217729.0 * c
    hi = t - (t - c)
    return hi, c - hi


def _cf(u):
    """P_1, P_2, P_3 of the continued fraction of Mills' ratio in u = 1 / x^2 (csrc/mes_math.h: mes_cf)."""
    b = np.ones_like(u)
    a = CF_K * u + 1.0
    for k in range(CF_K - 1, 1, -1):
        a, b = (k * u) * b + a, a
    return u * b + a, a, b


def mes_g(c):
    """g(c), elementwise; NaN -> NaN, +inf -> +0, -inf -> +inf.  The pieces and why: csrc/mes_math.h."""
    c = np.asarray(c, dtype=float)
    out = np.full(c.shape, np.nan)
    with np.errstate(all='ignore'):
        out[c >= ZERO] = 0.0
        m = (c >= FAR) & (c < ZERO)
        x = c[m]
        h = x * x
        hi, lo = _split(x)
        l = ((hi * hi - h) + 2.0 * hi * lo) + lo * lo          # c^2 - fl(c^2), exactly: the device's fma(c, c, -h)
        e2 = np.exp(-0.25 * h)
        t = 1.0 / x
        p1, p2, _ = _cf(t * t)
        a = INV_SQRT_2PI * (t * (p2 / p1) + 0.5 * x)
        a = a - 0.5 * l * a
        out[m] = (a * e2) * e2
        m = (c >= 0.0) & (c < FAR)
        x = c[m]
        h = x * x
        hi, lo = _split(x)
        l = ((hi * hi - h) + 2.0 * hi * lo) + lo * lo
        e = np.exp(-0.5 * h)
        phi = INV_SQRT_2PI * (e - 0.5 * l * e)
        Q = 0.5 * erfc(x * INV_SQRT2)
        out[m] = (0.5 * x) * phi / (1.0 - Q) - np.log1p(-Q)
        m = (c < 0.0) & (c >= -FAR)
        x = c[m]
        w = SQRT_HALF_PI * erfcx(-x * INV_SQRT2)
        out[m] = (0.5 * x) * (1.0 + x * w) / w + (HALF_LOG_2PI - np.log(w))
        m = c < -FAR
        x = -c[m]
        t = 1.0 / x
        _, p2, p3 = _cf(t * t)
        inv_d2 = p3 / p2
        out[m] = (HALF_LOG_2PI - 0.5 * inv_d2) + np.log(t * inv_d2 + x)
    return out


def mes_dg(c):
    """g'(c) = -(h / 2) (1 + c^2 + c h), h = phi / Phi = exp(log phi - log_ndtr(c))."""
    c = np.asarray(c, dtype=float)
    with np.errstate(all='ignore'):
        h = np.exp(-0.5 * c * c - HALF_LOG_2PI - log_ndtr(c))
        return -0.5 * h * (1.0 + c * c + c * h)


def _ystar(ystar):
    ystar = np.asarray(ystar, dtype=float).reshape(-1)
    if not 1 <= len(ystar) <= MAX_S or not np.all(np.isfinite(ystar)):
        raise ValueError('MES takes 1 to %d finite maximum samples' % MAX_S)
    return ystar


def mes_value(mu, s2, ystar):
    """MES at the moments (mu, s2) (M,) for the maxima ystar (S,): the sum in s ascending with its roundings carried along (TwoSum) and
    returned once, then one division -- the device's order (csrc/kernels_mes.hip: S equal samples give the bits of one)."""
    ystar = _ystar(ystar)
    mu, s = np.asarray(mu, dtype=float), np.sqrt(np.asarray(s2, dtype=float))
    acc = mes_g((ystar[0] - mu) / s)
    lost = np.zeros_like(acc)
    with np.errstate(invalid='ignore'):
        for y in ystar[1:]:
            g = mes_g((y - mu) / s)
            t = acc + g
            bv = t - acc
            lost = lost + ((acc - (t - bv)) + (g - bv))
            acc = t
        tot = acc + lost
    return np.where(np.isnan(tot), acc, tot) / float(len(ystar))


def mes_value_grad(mu, s2, dmu, ds2, ystar):
    """(MES (M,), dMES/dx (M, d)) from the moments and their gradients: dgamma/dx = -dmu / s - gamma ds2 / (2 s2)."""
    ystar = _ystar(ystar)
    mu, s2 = np.asarray(mu, dtype=float), np.asarray(s2, dtype=float)
    s = np.sqrt(s2)
    grad = np.zeros(np.shape(dmu))
    for y in ystar:
        c = (y - mu) / s
        grad = grad + mes_dg(c)[:, None] * (-dmu / s[:, None] - (0.5 * c / s2)[:, None] * ds2)
    return mes_value(mu, s2, ystar), grad / float(len(ystar))


GUMBEL_LEVELS = (0.25, 0.5, 0.75)


def gumbel_quantiles(mu, s, levels=GUMBEL_LEVELS):
    """The y at which P(max_i f_i <= y) = prod_i Phi((y - mu_i) / s_i) -- the support points taken as independent -- equals each
    level: bisection on sum_i log Phi to the last bit of y."""
    mu, s = np.asarray(mu, dtype=float), np.asarray(s, dtype=float)

    def logp(y):
        return float(np.sum(log_ndtr((y - mu) / s)))

    out = []
    for q in levels:
        target = np.log(q)
        lo, hi = float(np.min(mu - 5.0 * s)), float(np.max(mu + 5.0 * s))
        while logp(lo) > target:
            lo -= (hi - lo) + 1.0
        while logp(hi) < target:
            hi += (hi - lo) + 1.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if logp(mid) < target:
                lo = mid
            else:
                hi = mid
        out.append(hi)
    return np.array(out)


def sample_maxima(mu, s, nmax, floor, rng=None):
    """nmax maxima from the Gumbel approximation of the paper: the quartiles of the support's maximum fix location and scale,
        b = (q25 - q75) / (log log(4/3) - log log 4),   a = q50 + b log log 2,   y* = a - b log(-log u),  u ~ U(0, 1) from rng,
    floored at `floor` (the published implementation's rule: best mean at the data + xi + 5 sqrt(sn2))."""
    rng = rstate(rng)
    q25, q50, q75 = gumbel_quantiles(mu, s)
    b = (q25 - q75) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    a = q50 + b * np.log(np.log(2.0))
    u = rng.rand(int(nmax))
    with np.errstate(divide='ignore'):
        y = a - b * np.log(-np.log(u))
    y = np.where(np.isfinite(y), y, floor)          # (u = 0: the draw falls to the floor)
    return np.maximum(y, floor)
