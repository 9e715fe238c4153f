"""
Two-objective bookkeeping on the host (numpy only; maximisation, as everywhere in pybo): Pareto masks, the dominated hypervolume, the
strips of a front and the closed-form expected hypervolume improvement (EHVI; Emmerich et al. 2011, Yang et al. 2019) from posterior
moments.  `strips` is the Python twin of `ehvi_strips` and `ehvi_from_moments` restates `ehvi_value` / `ehvi_fold_term` of
csrc/ehvi_math.h statement for statement; the whole-grid evaluation is the device's (`gpx_ehvi_sweep`, `models.MultiObjective.acq_topk`).

A front of n points above the reference point r cuts the region it does not dominate into n + 1 vertical strips
[a_i, a_{i+1}) x [b_i, inf), i = 0 .. n, with a_0 = r1, a_i = f1 of point i (by f1 ascending), a_{n+1} = +inf, b_i = f2 of point i + 1
and b_n = r2:

    HVI(y) = sum_i [min(y1, a_{i+1}) - a_i]_+ [y2 - b_i]_+
    EHVI   = sum_i max(EI_1(a_i) - EI_1(a_{i+1}), 0) EI_2(b_i),    EI_j(t) = (mu_j - t) Phi(z) + s_j phi(z),  z = (mu_j - t) / s_j,  EI_1(inf) = 0
"""
import numpy as np
from scipy.special import erfc, erfcx

__all__ = ['pareto_mask', 'hypervolume', 'hv_contributions', 'strips', 'ehvi_from_moments', 'default_ref']


def _points(Y):
    Y = np.asarray(Y, dtype=float)
    return Y.reshape(-1, 2) if Y.size else np.empty((0, 2))


def pareto_mask(Y):
    """Boolean mask over the rows of Y (n, 2): True where no other row is at least as good in both coordinates and different; of equal
    rows the first one alone is kept."""
    Y = _points(Y)
    n = len(Y)
    keep = np.zeros(n, dtype=bool)
    # f1 descending, f2 descending, index ascending: a row survives exactly when its f2 exceeds every f2 met before it
    order = np.lexsort((np.arange(n), -Y[:, 1], -Y[:, 0]))
    best = -np.inf
    for i in order:
        if Y[i, 1] > best:
            keep[i] = True
            best = Y[i, 1]
    return keep


def strips(Y, ref):
    """(a (n + 2,), b (n + 1,)) of the raw points Y over the reference point ref: rows not strictly above ref in both coordinates, weakly
    dominated rows and duplicates are dropped; every entry is a copy of an input double (csrc/ehvi_math.h: ehvi_strips)."""
    Y = _points(Y)
    ref = np.asarray(ref, dtype=float).reshape(2)
    Y = Y[(Y[:, 0] > ref[0]) & (Y[:, 1] > ref[1])]
    Y = Y[pareto_mask(Y)]
    Y = Y[np.argsort(Y[:, 0], kind='stable')]
    a = np.concatenate([[ref[0]], Y[:, 0], [np.inf]])
    b = np.concatenate([Y[:, 1], [ref[1]]])
    return a, b


def hypervolume(Y, ref):
    """Area dominated by the rows of Y (n, 2) and bounded below by ref."""
    a, b = strips(Y, ref)
    ref = np.asarray(ref, dtype=float).reshape(2)
    # point i (1-based) adds the rectangle (a_{i-1}, a_i] x (r2, f2_i]
    return float(np.sum((a[1:-1] - a[:-2]) * (b[:-1] - ref[1])))


def hv_contributions(Y, ref):
    """Per row of Y: hypervolume(Y) - hypervolume(Y without that row) (0 for dominated rows, duplicates and rows not above ref)."""
    Y = _points(Y)
    total = hypervolume(Y, ref)
    out = np.zeros(len(Y))
    for i in range(len(Y)):
        out[i] = total - hypervolume(np.delete(Y, i, axis=0), ref)
    return np.maximum(out, 0.0)


def default_ref(F):
    """The reference point the EHVI policy and the Pareto recommender share: F.min(0) - 0.1 span, span = F.max(0) - F.min(0), 1 where 0."""
    F = _points(F)
    lo, hi = F.min(0), F.max(0)
    span = hi - lo
    span[span == 0.0] = 1.0
    return lo - 0.1 * span


_RSQRT2 = 0.70710678118654752440
_RSQRT2PI = 0.39894228040143267794
_SQRT_HALF_PI = 1.25331413731550025121
_TAIL = -6.0


def _ei_parts(mu, s, t):
    """(EI, Phi(z), phi(z)) of N(mu, s^2) over t.  Below z = -6 the tail form EI = s phi(z) (1 + z sqrt(pi / 2) erfcx(-z / sqrt 2)): the plain
    form loses every digit once Phi(z) and phi(z) fall below the smallest normal double (z < -37.5), by factors of a thousand, and such an
    EI_2 is multiplied by an EI_1 that may be large."""
    with np.errstate(invalid='ignore', over='ignore', divide='ignore', under='ignore'):
        dlt = mu - t
        z = dlt / s
        pdf = _RSQRT2PI * np.exp(-0.5 * z * z)
        tail = (z < _TAIL) & (pdf > 0.0)          # (phi underflowed to 0: the plain form gives the 0 the tail form would)
        zt = np.where(tail, z, _TAIL)
        mills = _SQRT_HALF_PI * erfcx(-zt * _RSQRT2)          # Phi(z) / phi(z)
        cdf = np.where(tail, pdf * mills, 0.5 * erfc(-z * _RSQRT2))
        return np.where(tail, (s * pdf) * (1.0 + zt * mills), dlt * cdf + s * pdf), cdf, pdf


def ehvi_from_moments(mu1, s2_1, mu2, s2_2, a, b, grad_terms=None):
    """EHVI of independent normals N(mu_j, s2_j) (arrays (M,)) over the strips (a, b), the device's statements in the device's order: the
    sum starts at +0.0, the strips are added for i = 0 .. n, the clamp is `w < 0 ? 0 : w` (a NaN stays).  grad_terms = (dmu1, ds2_1, dmu2,
    ds2_2), each (M, d): returns (value, gradient (M, d)) by the product rule (dEI/dmu = Phi, dEI/ds2 = phi / (2 s))."""
    mu1, s2_1, mu2, s2_2 = (np.atleast_1d(np.asarray(v, dtype=float)) for v in (mu1, s2_1, mu2, s2_2))
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    n = len(b) - 1
    s1, s2 = np.sqrt(s2_1), np.sqrt(s2_2)
    acc = np.zeros(mu1.shape)
    grad = grad_terms is not None
    if grad:
        g_mu1, g_v1, g_mu2, g_v2 = (np.zeros(mu1.shape) for _ in range(4))
    e_prev, c_prev, p_prev = _ei_parts(mu1, s1, a[0])
    zero = np.zeros(mu1.shape)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n + 1):
            e_next, c_next, p_next = _ei_parts(mu1, s1, a[i + 1]) if i < n else (zero, zero, zero)
            e2, c2, p2 = _ei_parts(mu2, s2, b[i])
            dif = e_prev - e_next
            w = np.where(dif < 0.0, 0.0, dif)
            acc = acc + w * e2
            if grad:
                on = np.where(dif < 0.0, 0.0, 1.0)
                g_mu1 = g_mu1 + on * (c_prev - c_next) * e2
                g_v1 = g_v1 + on * (p_prev - p_next) * e2
                g_mu2 = g_mu2 + w * c2
                g_v2 = g_v2 + w * p2
            e_prev, c_prev, p_prev = e_next, c_next, p_next
    if not grad:
        return acc
    dmu1, dv1, dmu2, dv2 = (np.asarray(t, dtype=float) for t in grad_terms)
    g = (g_mu1[:, None] * dmu1 + (0.5 * g_v1 / s1)[:, None] * dv1 + g_mu2[:, None] * dmu2 + (0.5 * g_v2 / s2)[:, None] * dv2)
    return acc, g
