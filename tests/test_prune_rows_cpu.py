"""The second bound of a selection-only sweep without a GPU: on a small oracle model
(N = 512, 20000 candidates; oracle/gp_ref.py) with the row-block partials of q = colsum(V^2) added sequentially in float64, as
k_acq adds them, every prefix q_R over the leading R blocks gives

    EI((bias + dot) + delta, max(rho - q_R, 1e-100)) >= EI(mu, s2)

for every candidate -- exactly, but for the rounding of the two EI evaluations (devmath_ref.acq_bound, where a pair needs it) --
q_R is non-decreasing in R, q_nP is q, and the survivors of the cut at the k-th best value do not increase with R."""
import numpy as np
import scipy.linalg as sla
from scipy.special import erfc

import devmath_ref
from oracle import gp_ref
from helpers import synth_problem


def _ei(mu, s2, p0):
    """kernels_sweep.hip acq_value, EI, operation for operation in numpy."""
    s = np.sqrt(s2)
    dlt = mu - p0
    z = dlt / s
    return dlt * (0.5 * erfc(-z * 0.70710678118654752440)) + s * (0.39894228040143267794 * np.exp(-0.5 * z * z))


def test_every_row_prefix_bounds_the_variance_and_the_value():
    N, d, M, k = 512, 4, 20000, 10
    rho, bias, sn2 = 1.3, 0.2, 1.3e-3
    X, y, ell = synth_problem(N, d, seed=12)
    ell = ell * 0.6
    y = bias + np.sqrt(rho) * y
    Z = np.random.RandomState(112).rand(M, d)
    K = gp_ref.kernel(gp_ref.SE_ARD, X, X, ell, rho)
    K[np.diag_indices_from(K)] += sn2
    L = np.linalg.cholesky(K)
    T = sla.solve_triangular(L, np.eye(N), lower=True)
    a = T @ (y - bias)
    Ks = gp_ref.kernel(gp_ref.SE_ARD, X, Z, ell, rho)
    V = T @ Ks
    nP = N // 128
    Qp = np.stack([np.sum(V[b * 128:(b + 1) * 128] ** 2, axis=0) for b in range(nP)])
    Pp = np.stack([V[b * 128:(b + 1) * 128].T @ a[b * 128:(b + 1) * 128] for b in range(nP)])
    q, p = np.zeros(M), np.zeros(M)
    qR = []
    for b in range(nP):                     # k_acq's order, starting from 0.0
        q = q + Qp[b]
        p = p + Pp[b]
        qR.append(q.copy())
    mu, s2 = bias + p, np.fmax(rho - q, 1e-100)
    target = float(np.max(bias + K @ (T.T @ a) - sn2 * (T.T @ a)))
    acq = _ei(mu, s2, target)
    dot = Ks.T @ (T.T @ a)                  # the bound pass's row-dot
    S = float(np.sum(np.abs(T).T @ np.abs(a)))
    delta = gp_ref.prune_delta(S, N, rho, bias)
    assert np.all(np.abs((bias + dot) - mu) <= delta / 2)
    tau = acq[gp_ref.topk_desc(acq, k)[k - 1]]
    cut = tau * (1.0 - 1e-6)
    counts = [int(np.sum(~(_ei((bias + dot) + delta, np.full(M, rho), target) < cut)))]
    for R in range(1, nP + 1):
        assert np.all(Qp[R - 1] >= 0.0)
        if R > 1:
            assert np.all(qR[R - 1] >= qR[R - 2])           # adding a non-negative term never lowers a float sum
        s2R = np.fmax(rho - qR[R - 1], 1e-100)
        assert np.all(s2R >= s2)
        ub2 = _ei((bias + dot) + delta, s2R, target)
        low = np.flatnonzero((acq >= 1e-280) & ~(ub2 >= acq))
        assert len(low) <= 64, (R, len(low))
        for n in low:
            t1 = devmath_ref.acq_truth('ei', mu[n], s2[n], target)
            t2 = devmath_ref.acq_truth('ei', bias + dot[n] + delta, s2R[n], target)
            room = devmath_ref.acq_bound('ei', mu[n], s2[n], target, t1) + devmath_ref.acq_bound('ei', bias + dot[n] + delta, s2R[n], target, t2)
            assert ub2[n] + room >= acq[n], (R, n)
        surv = ~(ub2 < cut)
        assert np.all(surv[acq >= tau])                    # nobody who can reach the top-k is cut
        counts.append(int(surv.sum()))
    assert np.array_equal(np.fmax(rho - qR[-1], 1e-100), s2)
    assert all(c1 >= c2 for c1, c2 in zip(counts, counts[1:])), counts
    assert counts[0] > counts[-1] >= k, counts
    print('\nsurvivors of the cut by prefix length R = 0 .. %d: %s of %d' % (nP, counts, M))
