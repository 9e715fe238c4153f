"""Knowledge gradient of a finite set of lines on the host (numpy): the closure the CPU tests check against the 50-digit truth
(tests/kg_ref.py) and the arithmetic of pybo_amd/csrc/kg_math.h, which the device runs.

    KG = E_Z[max_j (a_j + b_j Z)] - max_j a_j,        Z ~ N(0, 1),  j = 0 .. n - 1

For a GP, a candidate z and a support set A: line 0 is (mu(z), s2(z) / D), line j is (mu(a_j), Sigma(a_j, z) / D), D = sqrt(s2(z) +
sn2) (`kg_lines`): the expected rise of the maximum posterior mean over {z} + A after one noisy observation at z (Frazier, Powell &
Dayanik 2009; Scott, Frazier & Powell 2011).

Form (kg_math.h): line j is the upper envelope on (lo_j, hi_j), lo_j the largest crossing with a flatter line, hi_j the smallest with
a steeper one; among equal slopes only the largest intercept counts (lowest index on a tie); then
    KG = sum_{j on} (b_j - b_0) (H(lo_j) - H(hi_j)),      H(c) = h(-|c|) = phi(|c|) - |c| (1 - Phi(|c|)),
Frazier's sum over the crossings regrouped per line.  No sort; O(n^2) per set."""
import numpy as np
from scipy.special import erfc

__all__ = ['kg_H', 'kg_intervals', 'kg_value', 'kg_value_grad', 'kg_lines', 'member_mean', 'KG_MAX_SUPPORT']

KG_MAX_SUPPORT = 127
_INV_SQRT2 = 0.70710678118654752440
_INV_SQRT_2PI = 0.39894228040143267794
_FAR, _CF_K, _ZERO = 8.0, 16, 39.0


def kg_H(c):
    """H(c) = h(-|c|), tail-stable: phi - x Q below x = 8, Mills' ratio by its continued fraction beyond (1 - x R = u P_3 / P_1,
    a quotient of positive terms), +0 from 39 on (and at +-inf)."""
    x = np.abs(np.asarray(c, dtype=float))
    out = np.zeros(x.shape)
    near = x < _FAR
    far = (x >= _FAR) & (x < _ZERO)

    def phi_parts(v):
        # exp(-v^2 / 2) with the rounding of v^2 put back (the header's FMA, here by Veltkamp's split): h2 + l = v^2 exactly
        h2 = v * v
        t = 134217729.0 * v
        vh = t - (t - v)
        vl = v - vh
        return h2, ((vh * vh - h2) + 2.0 * vh * vl) + vl * vl

    xn = x[near]
    h2, l = phi_parts(xn)
    e = np.exp(-0.5 * h2)
    out[near] = _INV_SQRT_2PI * (e - 0.5 * l * e) - xn * (0.5 * erfc(xn * _INV_SQRT2))
    xf = x[far]
    h2, l = phi_parts(xf)
    u = 1.0 / h2
    b, a = np.ones_like(u), 1.0 + _CF_K * u
    for k in range(_CF_K - 1, 1, -1):
        b, a = a, a + k * u * b
    p1 = a + u * b
    v = _INV_SQRT_2PI * (u * (b / p1))
    e2 = np.exp(-0.25 * h2)
    out[far] = ((v - 0.5 * l * v) * e2) * e2
    return out


def kg_intervals(alpha, beta):
    """(lo, hi, on) of every line: alpha, beta (..., n).  on[.., j]: line j is part of the upper envelope (hi > lo and not hidden
    behind a line of the same slope)."""
    a = np.asarray(alpha, dtype=float)
    b = np.asarray(beta, dtype=float)
    n = a.shape[-1]
    aj, ai = a[..., :, None], a[..., None, :]
    bj, bi = b[..., :, None], b[..., None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        c = (ai - aj) / (bj - bi)
    flatter, steeper, same = bi < bj, bi > bj, bi == bj
    lo = np.where(flatter, c, -np.inf).max(axis=-1)
    hi = np.where(steeper, c, np.inf).min(axis=-1)
    idx = np.arange(n)
    earlier = idx[None, :] < idx[:, None]                      # [j, i]: i < j
    hidden = (same & ((ai > aj) | ((ai == aj) & earlier))).any(axis=-1)
    return lo, hi, (~hidden) & (hi > lo)


def kg_value(alpha, beta, chunk=2048):
    """KG of the line sets alpha, beta (..., n) -> (...,)."""
    a = np.asarray(alpha, dtype=float)
    b = np.asarray(beta, dtype=float)
    shape = a.shape[:-1]
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    out = np.empty(len(a2))
    for i in range(0, len(a2), chunk):
        aa, bb = a2[i:i + chunk], b2[i:i + chunk]
        lo, hi, on = kg_intervals(aa, bb)
        terms = np.where(on, (bb - bb[:, :1]) * (kg_H(lo) - kg_H(hi)), 0.0)
        out[i:i + chunk] = np.maximum(terms.sum(axis=-1), 0.0)
    return out.reshape(shape)


def kg_value_grad(alpha, beta, dalpha0, dbeta):
    """Value and gradient: alpha, beta (M, n); dalpha0 (M, d) the gradient of line 0's intercept (the support lines' intercepts do
    not move with the candidate); dbeta (M, n, d).  With P_j = Phi(hi_j) - Phi(lo_j) and w_j = phi(lo_j) - phi(hi_j),
        dKG = (P_0 - [0 = argmax a]) da_0 + sum_j w_j db_j."""
    a = np.asarray(alpha, dtype=float)
    b = np.asarray(beta, dtype=float)
    lo, hi, on = kg_intervals(a, b)
    val = np.maximum(np.where(on, (b - b[:, :1]) * (kg_H(lo) - kg_H(hi)), 0.0).sum(axis=-1), 0.0)
    Phi = lambda c: 0.5 * erfc(-c * _INV_SQRT2)
    phi = lambda c: _INV_SQRT_2PI * np.exp(-0.5 * c * c)
    P0 = np.where(on[:, 0], Phi(hi[:, 0]) - Phi(lo[:, 0]), 0.0)
    w = np.where(on, phi(lo) - phi(hi), 0.0)
    top = (a[:, :1] >= a).all(axis=-1)
    g = (P0 - top)[:, None] * np.asarray(dalpha0, dtype=float) + np.einsum('mj,mjd->md', w, np.asarray(dbeta, dtype=float))
    return val, g


def kg_lines(mu, s2, sn2, mu_support, cov_support):
    """The lines of M candidates: mu, s2 (M,) their latent moments, mu_support (m,), cov_support (M, m) = Sigma(a_j, z).
    Returns alpha, beta (M, m + 1), line 0 the candidate's own."""
    mu = np.asarray(mu, dtype=float)
    s2 = np.asarray(s2, dtype=float)
    D = np.sqrt(s2 + sn2)
    alpha = np.column_stack([mu, np.broadcast_to(np.asarray(mu_support, dtype=float), (len(mu), len(mu_support)))])
    beta = np.column_stack([s2 / D, np.asarray(cov_support, dtype=float) / D[:, None]])
    return alpha, beta


def member_mean(outs):
    """The ensemble's value: the members' arrays summed in member order and divided once."""
    tot = np.array(outs[0], dtype=float)
    for o in outs[1:]:
        tot = tot + o
    return tot / len(outs)
