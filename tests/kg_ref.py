"""Oracle of the knowledge gradient (GPX_ACQ_KG; pybo_amd/csrc/kg_math.h, kernels_kg.hip).

  * fp64 numpy GP algebra on oracle.gp_ref.GPRef: the lines of candidates over a support set, and the analytic gradient;
  * kg_truth(alpha, beta): mpmath at 50 digits AT THE DOUBLES CONSUMED -- lines sorted by slope, the exact upper envelope (equal slopes:
    the largest intercept, the lowest index on a tie), Frazier's sum with h by mpmath; an independent algorithm (sort + stack), not
    the per-line form the code under test uses;
  * kg_bound(alpha, beta): the error bound kg_math.h derives, evaluated on the exact envelope;
  * two mutations the tests must be able to see: dropping line 0, and a padding line (0, 0)."""
import numpy as np
import mpmath as mp
import scipy.linalg as sla

from oracle import gp_ref

mp.mp.dps = 50
EPS = 2.0 ** -53
KG_H_REL = 7200.0 * EPS          # kg_math.h


def _h(c):
    """h(c) = phi(c) + c Phi(c), for c <= 0 (50 digits: the sum cancels c^2-fold, three digits at c = -38).  Below c = -1000 the
    value is under 1e-217000, zero for every double it multiplies."""
    if c < -1000:
        return mp.mpf(0)
    return mp.npdf(c) + c * mp.ncdf(c)


def envelope(alpha, beta):
    """The exact upper envelope of the lines a_j + b_j z: [(index, lo, hi)] by slope ascending, lo / hi mpmath numbers or -+inf."""
    a = [mp.mpf(float(x)) for x in alpha]
    b = [mp.mpf(float(x)) for x in beta]
    order = sorted(range(len(a)), key=lambda j: (b[j], -a[j], j))
    keep = []
    for j in order:                                  # equal slopes: the first in this order (largest intercept, lowest index)
        if keep and b[keep[-1]] == b[j]:
            continue
        keep.append(j)
    stack, start = [], []                            # lines of the envelope and where each one starts
    for j in keep:
        while stack:
            i = stack[-1]
            c = (a[i] - a[j]) / (b[j] - b[i])
            if c <= start[-1]:
                stack.pop()
                start.pop()
            else:
                break
        if stack:
            i = stack[-1]
            start.append((a[i] - a[j]) / (b[j] - b[i]))
        else:
            start.append(-mp.inf)
        stack.append(j)
    return [(stack[i], start[i], start[i + 1] if i + 1 < len(stack) else mp.inf) for i in range(len(stack))]


def kg_truth(alpha, beta, as_float=True):
    """E max_j (a_j + b_j Z) - max_j a_j at 50 digits: sum over the envelope's crossings of (b_next - b_this) h(-|c|)."""
    b = [mp.mpf(float(x)) for x in beta]
    env = envelope(alpha, beta)
    tot = mp.mpf(0)
    for (i, _, hi), (k, _, _) in zip(env[:-1], env[1:]):
        tot += (b[k] - b[i]) * _h(-abs(hi))
    return float(tot) if as_float else tot


def kg_bound(alpha, beta):
    """kg_math.h: |computed - truth| <= (KG_H_REL + (n + 4) eps) T + 2.04 eps n S + n 2^-1022, d_j = |b_j - b_0|, S = max d_j,
    T = sum over the exact envelope of d_j (H(lo_j) + H(hi_j))."""
    b = np.asarray(beta, dtype=float)
    n = len(b)
    b0 = mp.mpf(float(b[0]))
    T = mp.mpf(0)
    for j, lo, hi in envelope(alpha, beta):
        dj = abs(mp.mpf(float(b[j])) - b0)
        T += dj * ((_h(-abs(lo)) if lo != -mp.inf else 0) + (_h(-abs(hi)) if hi != mp.inf else 0))
    S = float(np.max(np.abs(b - b[0])))
    return float((KG_H_REL + (n + 4) * EPS) * T) + 2.04 * EPS * n * S + n * 2.0 ** -1022


def drop_line0(alpha, beta):
    """MUTATION: the candidate's own line left out."""
    return np.asarray(alpha)[..., 1:], np.asarray(beta)[..., 1:]


def add_padding_line(alpha, beta):
    """MUTATION: a padding column (m < 127) taken for a line (0, 0)."""
    a, b = np.asarray(alpha, dtype=float), np.asarray(beta, dtype=float)
    z = np.zeros(a.shape[:-1] + (1,))
    return np.concatenate([a, z], axis=-1), np.concatenate([b, z], axis=-1)


# ---- GP algebra ------------------------------------------------------------------------------------------------------
def make_model(X, y, kernel, ell, rho, sn2, bias):
    m = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    m.add_data(X, y)
    return m


def lines(model, A, Z, grad=False):
    """alpha, beta (M, m + 1) of the candidates Z over the support set A; with grad also dalpha0 (M, d), dbeta (M, m + 1, d)."""
    A = np.array(A, ndmin=2, dtype=float)
    Z = np.array(Z, ndmin=2, dtype=float)
    kid, ell, rho = model.kid, model.ell, model.rho
    post = model.predict(Z, grad=grad)
    mu, s2 = post[:2]
    muA = model.predict(A)[0]
    KA = gp_ref.kernel(kid, model.X, A, ell, rho)                          # (N, m)
    B = sla.cho_solve((model.L, True), KA)                                 # (K + sn2 I)^-1 k(X, A)
    KZ = gp_ref.kernel(kid, model.X, Z, ell, rho)                          # (N, M)
    cov = gp_ref.kernel(kid, Z, A, ell, rho) - KZ.T @ B                    # Sigma(a_j, z) (M, m)
    D = np.sqrt(s2 + model.sn2)
    alpha = np.column_stack([mu, np.broadcast_to(muA, (len(Z), len(A)))])
    beta = np.column_stack([s2 / D, cov / D[:, None]])
    if not grad:
        return alpha, beta
    dmu, ds2 = post[2:]
    d = Z.shape[1]
    Zs, As, Xs = Z / ell, A / ell, model.X / ell
    GA = gp_ref.dkern_dr2(kid, gp_ref.sqdist(Zs, As), rho)                 # (M, m)
    GX = gp_ref.dkern_dr2(kid, gp_ref.sqdist(Xs, Zs), rho)                 # (N, M)
    dbeta = np.empty((len(Z), len(A) + 1, d))
    dbeta[:, 0, :] = ds2 * (1.0 / D - s2 / (2.0 * D ** 3))[:, None]
    for t in range(d):
        dkA = GA * (2.0 * (Zs[:, t][:, None] - As[:, t][None, :]) / ell[t])            # d/dz_t k(z, a_j)
        dkX = GX * (2.0 * (Zs[:, t][None, :] - Xs[:, t][:, None]) / ell[t])            # d/dz_t k(z, x_n) (N, M)
        dcov = dkA - dkX.T @ B
        dbeta[:, 1:, t] = dcov / D[:, None] - beta[:, 1:] * (ds2[:, t] / (2.0 * D * D))[:, None]
    return alpha, beta, dmu, dbeta


def kg_oracle(model, A, Z):
    """The oracle's value at every candidate: the 50-digit truth at the oracle's own lines."""
    alpha, beta = lines(model, A, Z)
    return np.array([kg_truth(a, b) for a, b in zip(alpha, beta)]), alpha, beta


def kg_oracle_grad(model, A, Z):
    from pybo_amd.kg import kg_value_grad
    alpha, beta, dmu, dbeta = lines(model, A, Z, grad=True)
    return kg_value_grad(alpha, beta, dmu, dbeta)


def value_tol(model, alpha, beta, rho):
    """The parity tolerance of a device value against the oracle, from the stated moment tolerances (tests/helpers.py) and
    no new number: KG is 1-Lipschitz in each intercept and the max term adds another: 2 max_j |d alpha_j|; it is E|Z| = 0.8-Lipschitz
    in the slopes: 0.8 max_j |d beta_j|.  d alpha from the mean tolerance; d beta from the s2 tolerance applied to the covariance
    (cov = beta D) and to s2 inside D, to first order: d beta_j = d cov_j / D + |beta_j| d s2 / (2 D^2)."""
    from helpers import mu_tol, s2_tol
    alpha, beta = np.asarray(alpha), np.asarray(beta)
    b0 = beta[:, 0]
    s2 = (b0 ** 2 + np.sqrt(b0 ** 4 + 4.0 * b0 ** 2 * model.sn2)) / 2.0          # from b_0 = s2 / sqrt(s2 + sn2)
    D2 = s2 + model.sn2
    D = np.sqrt(D2)
    dalpha = np.max(mu_tol(alpha, rho), axis=1)
    cov = beta * D[:, None]
    dcov = s2_tol(cov, rho)
    dbeta = np.max(dcov / D[:, None] + np.abs(beta) * s2_tol(s2, rho)[:, None] / (2.0 * D2[:, None]), axis=1)
    return 2.0 * dalpha + 0.8 * dbeta
