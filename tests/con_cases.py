"""The small constrained problems shared by test_con_cpu.py (the oracle's survivor count) and test_gpu_constrained.py (DESIGN.md
section 2.3).  The smallest shapes at which the selection-only constrained sweep can go wrong: N = 300 is three block rows and
N = 1100 nine, so a generation is G = 4096 candidates and pruning is legal from M = 3 G = 12288; M = 13001 is off the tile grid.
Objective: helpers.synth_problem; constraint j: c_j = cos(2 sum(x) + j) + 0.3 sin(4 x[(j+1) % d]) + noise, feasible where c_j is at
least its median over the observations.  The objective takes ens_prune_cases.HYPERS[0], constraint j takes HYPERS[1 + j]."""
import numpy as np

from helpers import synth_problem
from ens_prune_cases import HYPERS, KS, G, M, cap_of      # noqa: F401 (shared with the tests)

# (N, d, kernel, seed, J)
CASES = {
    'se_j2': (300, 8, 'se', 14, 2),
    'm5_j3': (300, 6, 'matern5', 12, 3),
    'se_j1': (300, 7, 'se', 13, 1),
    'se_j2_n9': (1100, 8, 'se', 15, 2),
}


def constraint_data(X, seed, J):
    """(N, J) noisy constraint observations at the rows of X."""
    d = X.shape[1]
    return np.column_stack([np.cos(2.0 * X.sum(1) + j) + 0.3 * np.sin(4.0 * X[:, (j + 1) % d]) + 1e-2 * np.random.RandomState(seed + 7 + j).randn(len(X))
                            for j in range(J)])


def build(N, d, kernel, seed, J, m=M):
    """dict(X, y, C (N, J), thr (J,), Z (m, d), hypers [(sn2, rho, ell (d,), bias)] of the objective and the J constraints, target =
    the best y among the feasible observations)."""
    X, y, ell = synth_problem(N, d, seed=seed)
    C = constraint_data(X, seed, J)
    thr = np.median(C, axis=0)
    Z = np.random.RandomState(seed + 100).rand(m, d)
    hypers = [(sn2, rho, ell * f, bias) for sn2, rho, f, bias in HYPERS[:1 + J]]
    feasible = np.all(C >= thr, axis=1)
    return dict(N=N, d=d, kernel=kernel, seed=seed, J=J, X=X, y=y, C=C, thr=thr, Z=Z, hypers=hypers, target=float(np.max(y[feasible])))


def problem(name, m=M):
    return build(*CASES[name], m=m)
