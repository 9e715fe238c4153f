"""The joint posterior at a point set on the CPU oracle, and the cases tests/test_gpu_joint.py runs (computed once per session).

    Sigma_ref = k(Z, Z) - V^T V,  V = solve_triangular(L, k(X, Z)),  mu_ref = predict(Z)[0]

Default problem of the issue: X, Z ~ U[0, 1]^d, y = sin(3 sum x) + 0.01 noise, rho = 1.7, bias = 0.4, sn2 = 1e-4.  The shapes are
the smallest that reach every branch of the device code: N = 300 is three padded block rows; M = 1, 5 sit inside one tile, 128 fills
it, 257 gives diagonal tiles, off-diagonal tiles and a ragged last panel; d = 40 walks the coordinates past the cross-Gram's
16-coordinate stage and the 32-coordinate slab; the appended cases cross no / one block boundary; N = 4224 is 33 block rows.
The length-scales keep the squared scaled distances of the d = 3, ell = 0.3 case (ell grows like sqrt(d)), so that the data
explain a comparable share of the variance in every case."""
import functools

import numpy as np
import scipy.linalg as sla

from oracle import gp_ref

RHO, BIAS, SN2 = 1.7, 0.4, 1e-4
KERNELS = ('se', 'matern5', 'matern3', 'matern1')

# tag -> (N, d, M, kernel, ell, appended observations)
CASES = {}
for _k in KERNELS:
    for _m in (1, 5, 128, 257):
        CASES['%s_m%d' % (_k, _m)] = (300, 3, _m, _k, 0.3, 0)
CASES['n513_d8_m384'] = (513, 8, 384, 'se', 0.5, 0)
CASES['d40'] = (300, 40, 257, 'matern5', 1.1, 0)
CASES['append_300'] = (300, 3, 257, 'matern5', 0.3, 1)          # 300 -> 301: inside the last block
CASES['append_384'] = (384, 3, 257, 'se', 0.3, 1)               # 384 -> 385: adds a block
CASES['n4224_m384'] = (4224, 8, 384, 'matern5', 0.5, 0)         # 33 block rows


def problem(N, d, M, seed=0, extra=0):
    """X (N + extra, d), y, Z (M, d) of the default problem (the last `extra` observations are the ones a test appends)."""
    rng = np.random.RandomState(seed)
    X = rng.rand(N + extra, d)
    y = np.sin(3.0 * X.sum(1)) + 0.01 * rng.randn(N + extra)
    Z = rng.rand(M, d)
    return X, y, Z


def joint(ref, Z):
    """(mu_ref, Sigma_ref) of a fitted oracle model at the rows of Z."""
    Ks = gp_ref.kernel(ref.kid, ref.X, Z, ref.ell, ref.rho)
    V = sla.solve_triangular(ref.L, Ks, lower=True)
    Sigma = gp_ref.kernel(ref.kid, Z, Z, ref.ell, ref.rho) - V.T @ V
    return ref.predict(Z)[0], Sigma


@functools.lru_cache(maxsize=None)
def case(tag):
    """dict(X, y, Z, d, kernel, ell, nappend, mu, Sigma): the problem and the oracle's joint posterior on ALL its observations.
    Shared by the tests of a session: treat the arrays as read-only."""
    N, d, M, kernel, ell, nappend = CASES[tag]
    X, y, Z = problem(N, d, M, seed=len(tag) + N + M, extra=nappend)
    ell = np.full(d, float(ell))
    ref = gp_ref.make_gp(SN2, RHO, ell, BIAS, kernel)
    ref.add_data(X, y)
    mu, Sigma = joint(ref, Z)
    for a in (X, y, Z, mu, Sigma):
        a.setflags(write=False)
    return dict(X=X, y=y, Z=Z, d=d, kernel=kernel, ell=ell, nappend=nappend, mu=mu, Sigma=Sigma)


def cov_tol(Sigma_ref, rho=RHO):
    """The variance tolerance of DESIGN.md section 6 carried to off-diagonal entries by Cauchy-Schwarz."""
    dg = np.maximum(np.diag(Sigma_ref), 0.0)
    return 1e-6 * np.sqrt(np.outer(dg, dg)) + 1e-10 * rho
