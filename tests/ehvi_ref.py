"""Reference maths of the two-objective index on the float64 oracle (oracle/gp_ref.py), written from the
definitions and independent of pybo_amd/pareto.py.  Test infrastructure: nothing under pybo_amd/ imports it.

    front:  the points strictly above r that no other point weakly dominates, one copy each, by f1 ascending
    HV(P):  the area of the union of the boxes [r, p], by the sweep over the front
    HVI(y) = HV(P + {y}) - HV(P) = sum_i [min(y1, a_{i+1}) - a_i]_+ [y2 - b_i]_+          (the strips; checked in test_ehvi_cpu.py)
    EHVI   = sum_i max(EI_1(a_i) - EI_1(a_{i+1}), 0) EI_2(b_i)                           (independent normals; checked by Monte Carlo)

Tolerances.  S = sum_i (|EI_1(a_i)| + |EI_1(a_{i+1})|) |EI_2(b_i)| bounds the magnitude of what the sum cancels in w_i; TINY, the smallest
normal double, is added for values in the subnormal range (con_ref.py).  End to end the library states its moments to mu_tol and s2_tol
(tests/helpers.py): each of the four oracle moments is moved by its tolerance, one at a time, the absolute changes of the closed form are
added and multiplied by 1.05, then 1e-6 S + TINY."""
import numpy as np

from oracle import gp_ref
from helpers import mu_tol, s2_tol

TINY = float(np.finfo(np.float64).tiny)


def front(P, r):
    """The non-dominated points of P (np, 2) strictly above r, one copy each, by f1 ascending -- by the definition (quadratic)."""
    P = np.asarray(P, dtype=float).reshape(-1, 2)
    P = np.unique(P[(P[:, 0] > r[0]) & (P[:, 1] > r[1])], axis=0)          # (sorted by f1, then f2; one copy each)
    keep = [p for p in P if not any(q[0] >= p[0] and q[1] >= p[1] and (q[0] != p[0] or q[1] != p[1]) for q in P)]
    return np.array(keep).reshape(-1, 2)


def strips(P, r):
    F = front(P, r)
    return np.concatenate([[r[0]], F[:, 0], [np.inf]]), np.concatenate([F[:, 1], [r[1]]])


def hypervolume(P, r):
    """Area of the union of the boxes [r, p]: the front from the right, each point adding the slab its f2 rises above the best so far."""
    F = front(P, r)
    area, top = 0.0, r[1]
    for f1, f2 in F[::-1]:
        area += (f1 - r[0]) * (f2 - top)
        top = f2
    return area


def hvi_strips(y, a, b):
    y = np.asarray(y, dtype=float).reshape(-1, 2)
    w = np.maximum(np.minimum(y[:, :1], a[None, 1:]) - a[None, :-1], 0.0)
    return np.sum(w * np.maximum(y[:, 1:] - b[None, :], 0.0), axis=1)


def ei(mu, s, t):
    """EI of N(mu, s^2) over t: the oracle's form (gp_ref.norm_cdf / norm_pdf); below z = -6 the tail form s phi(z) (1 + z M(z)) with the
    Mills ratio M = sqrt(pi / 2) erfcx(-z / sqrt 2).  Checked against 60-digit arithmetic: the plain form is off by a factor 1400 at z = -38,
    where Phi and phi are subnormal, the tail form by 2e-13 -- and an EI down there is multiplied by the other objective's, which may be 100."""
    from scipy.special import erfcx
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        z = (mu - t) / s
        tail = (z < -6.0) & (gp_ref.norm_pdf(z) > 0.0)
        zt = np.where(tail, z, -6.0)
        far = (s * gp_ref.norm_pdf(z)) * (1.0 + zt * (1.25331413731550025121 * erfcx(-zt * 0.70710678118654752440)))
        return np.where(tail, far, (mu - t) * gp_ref.norm_cdf(z) + s * gp_ref.norm_pdf(z))


def terms(mu1, s2_1, mu2, s2_2, a, b):
    """(E1 (M, n + 2) with the last column 0, E2 (M, n + 1))"""
    mu1, s2_1, mu2, s2_2 = (np.atleast_1d(np.asarray(v, dtype=float)) for v in (mu1, s2_1, mu2, s2_2))
    E1 = np.column_stack([ei(mu1[:, None], np.sqrt(s2_1)[:, None], a[None, :-1]), np.zeros(len(mu1))])
    E2 = ei(mu2[:, None], np.sqrt(s2_2)[:, None], b[None, :])
    return E1, E2


def ehvi(mu1, s2_1, mu2, s2_2, a, b):
    E1, E2 = terms(mu1, s2_1, mu2, s2_2, a, b)
    with np.errstate(invalid='ignore'):
        return np.sum(np.maximum(E1[:, :-1] - E1[:, 1:], 0.0) * E2, axis=1)


def magnitude(mu1, s2_1, mu2, s2_2, a, b):
    """S of the module's docstring."""
    E1, E2 = terms(mu1, s2_1, mu2, s2_2, a, b)
    with np.errstate(invalid='ignore'):
        return np.sum((np.abs(E1[:, :-1]) + np.abs(E1[:, 1:])) * np.abs(E2), axis=1)


def fit(hyper, kernel, X, y):
    sn2, rho, ell, bias = hyper
    r = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    r.add_data(X, y)
    return r


def models(p, n=None):
    """The oracle's two objective models of an ehvi_cases problem (the first n observations)."""
    n = len(p['X']) if n is None else n
    return [fit(p['hypers'][j], p['kernels'][j], p['X'][:n], p['Y'][:n, j]) for j in range(2)]


def values(ms, a, b, Z):
    """(EHVI, its end-to-end tolerance, the four moments) at the rows of Z from the oracle models ms."""
    moms = []
    for m in ms:
        mu, s2 = m.predict(Z)
        moms += [mu, s2]
    v = ehvi(*moms, a, b)
    tol = np.zeros_like(v)
    deltas = [mu_tol(moms[0], ms[0].rho), s2_tol(moms[1], ms[0].rho), mu_tol(moms[2], ms[1].rho), s2_tol(moms[3], ms[1].rho)]
    for q in range(4):
        moved = list(moms)
        moved[q] = moved[q] + deltas[q]
        tol += np.abs(ehvi(*moved, a, b) - v)
    return v, 1.05 * tol + 1e-6 * magnitude(*moms, a, b) + TINY, moms
