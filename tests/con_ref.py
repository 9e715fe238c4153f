"""Reference maths of the constrained index on the float64 oracle (oracle/gp_ref.py).  Test infrastructure:
nothing under pybo_amd/ imports it.

    v_0 = a (EI or PI of the objective),  v_j = fold(v_{j-1}, P_j),  P_j = Pr(c_j >= thr_j) = Phi((mu_j - thr_j) / s_j)
    w_1 = fold(1, P_1),  w_j = fold(w_{j-1}, P_j)                     fold(v, p) = v * min(p, 1)   (csrc/acq_core.h: con_fold)

Tolerances.  The library states its moments to mu_tol and s2_tol (tests/helpers.py) and EI to ei_tol, those two propagated to first
order.  The same propagation through P = Phi(z), z = (mu - t) / s (dP/dmu = phi(z) / s, dP/ds2 = -z phi(z) / (2 s2)) gives pi_tol;
through the product v = a prod_j P_j, with every P_j <= 1 and every factor's error independent,

    |dv| <= da prod_j P_j + a sum_j dP_j prod_{i != j} P_i  <=  da + a sum_j dP_j                (first order)

The right-hand form is used: it needs no division by a P_j that may be 0, and it is the looser of the two only by factors P <= 1.
For the probability of feasibility alone a = 1 and da = 0.

Below the smallest normal double (2.2e-308) a value has no relative precision left: a subnormal carries fewer than 53 bits, and an
EI or PI of the objective 38 standard deviations below the target lands there through exp() of the tail, where one implementation
returns 4e-313 and the next 3e-316 or 0.  TINY = that number is therefore added to every tolerance: an absolute term, 300 orders of
magnitude below anything a top-k can tell apart."""
import numpy as np

from oracle import gp_ref
from helpers import ei_tol, mu_tol, s2_tol

TINY = float(np.finfo(np.float64).tiny)


def fold(v, p):
    with np.errstate(invalid='ignore'):
        return v * np.minimum(p, 1.0)             # (np.minimum keeps a NaN p)


def chain(a, ps):
    """v_J from v_0 = a and the factors in order."""
    v = a
    for p in ps:
        v = fold(v, p)
    return v


def pof_chain(ps):
    return chain(1.0, ps)


def fit(hyper, kernel, X, y):
    sn2, rho, ell, bias = hyper
    r = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    r.add_data(X, y)
    return r


def models(p, n=None):
    """The oracle's objective and constraint models of a con_cases problem (the first n observations)."""
    n = len(p['X']) if n is None else n
    obj = fit(p['hypers'][0], p['kernel'], p['X'][:n], p['y'][:n])
    cons = [fit(p['hypers'][1 + j], p['kernel'], p['X'][:n], p['C'][:n, j]) for j in range(p['J'])]
    return obj, cons


def pi_from_moments(mu, s2, t):
    return gp_ref.norm_cdf((mu - t) / np.sqrt(s2))


def pi_tol(mu, s2, t, rho):
    s = np.sqrt(s2)
    z = (mu - t) / s
    pdf = gp_ref.norm_pdf(z)
    return 1e-6 * gp_ref.norm_cdf(z) + 1.05 * (pdf / s * mu_tol(mu, rho) + np.abs(z) * pdf / (2.0 * s2) * s2_tol(s2, rho))


def values(obj, cons, thr, acq, target, Z):
    """(v_J, w_J, tolerance of v_J, tolerance of w_J) at the rows of Z; acq 'ei', 'pi' or None (no objective: v_J = w_J)."""
    ps, dps = [], []
    for c, t in zip(cons, thr):
        mu, s2 = c.predict(Z)
        ps.append(pi_from_moments(mu, s2, t))
        dps.append(pi_tol(mu, s2, t, c.rho))
    w = pof_chain(ps)
    dw = sum(dps) + TINY
    if acq is None:
        return w, w, dw, dw
    mu, s2 = obj.predict(Z)
    if acq == 'ei':
        a, da = obj.get_improvement(target, Z), ei_tol(mu, s2, target, obj.rho)
    else:
        a, da = pi_from_moments(mu, s2, target), pi_tol(mu, s2, target, obj.rho)
    return chain(a, ps), w, da + np.abs(a) * dw + TINY, dw


def value_grad(obj, cons, thr, target, X):
    """cEI (target None: the probability of feasibility) and its gradient at the rows of X, product rule over the oracle's
    get_improvement / get_tail gradients."""
    X = np.array(X, ndmin=2, dtype=float)
    if target is None:
        v, g = np.ones(len(X)), np.zeros(X.shape)
    else:
        v, g = obj.get_improvement(target, X, True)
    for c, t in zip(cons, thr):
        p, dp = c.get_tail(t, X, True)
        g = g * p[:, None] + v[:, None] * dp
        v = v * p
    return v, g


def value_grad_from_moments(moms, ts, has_obj):
    """(v, g) of the constrained index from the members' moments and their gradients: moms = [(mu, s2, dmu, ds2)] per member (the
    objective first where has_obj), ts the target / thresholds in the same order."""
    v = g = None
    for i, ((mu, s2, dmu, ds2), t) in enumerate(zip(moms, ts)):
        s = np.sqrt(s2)
        z = (mu - t) / s
        cdf, pdf = gp_ref.norm_cdf(z), gp_ref.norm_pdf(z)
        if has_obj and i == 0:
            f, df = (mu - t) * cdf + s * pdf, cdf[:, None] * dmu + (0.5 * pdf / s)[:, None] * ds2
        else:
            f, df = cdf, pdf[:, None] * (dmu / s[:, None] - (0.5 * z / s2)[:, None] * ds2)
        v, g = (f, df) if v is None else (v * f, g * f[:, None] + v[:, None] * df)
    return v, g


def grad_tol(models_, ts, has_obj, X):
    """First-order tolerance of the index's gradient at the rows of X: every input of value_grad_from_moments is moved by its stated
    tolerance, one at a time -- mu by mu_tol, s2 by s2_tol, every component of dmu and ds2 by 1e-6 relative + 1e-8 (the bound
    tests/test_gpu_parity.py holds predict's gradients to) -- and the absolute changes of the gradient are added up (x 1.05)."""
    moms = [m.predict(X, grad=True) for m in models_]
    g0 = value_grad_from_moments(moms, ts, has_obj)[1]
    tol = np.zeros_like(g0)
    for i, m in enumerate(models_):
        deltas = [mu_tol(moms[i][0], m.rho), s2_tol(moms[i][1], m.rho)]
        for q in (0, 1):
            moved = list(moms[i])
            moved[q] = moved[q] + deltas[q]
            tol += np.abs(value_grad_from_moments(moms[:i] + [tuple(moved)] + moms[i + 1:], ts, has_obj)[1] - g0)
        for q in (2, 3):
            for j in range(X.shape[1]):
                moved = [a.copy() for a in moms[i]]
                moved[q][:, j] += 1e-6 * np.abs(moved[q][:, j]) + 1e-8
                tol += np.abs(value_grad_from_moments(moms[:i] + [tuple(moved)] + moms[i + 1:], ts, has_obj)[1] - g0)
    return 1.05 * tol
