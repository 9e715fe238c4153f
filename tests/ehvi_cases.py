"""The small two-objective problems shared by test_ehvi_cpu.py and test_gpu_ehvi.py.  N = 300 is three block
rows, M = 13001 is off the tile grid.  Objective 1: helpers.synth_problem with the case's kernel and ens_prune_cases.HYPERS[0]; objective 2:
cos(2 sum(x)) + 0.3 sin(4 x_1) + noise -- it falls where the first rises over much of the box -- with the OTHER kernel and HYPERS[1]."""
import numpy as np

from helpers import synth_problem
from ens_prune_cases import HYPERS, M      # noqa: F401 (shared with the tests)

# name -> (N, d, kernel of objective 1, seed)
CASES = {
    'se_d8': (300, 8, 'se', 21),
    'm5_d6': (300, 6, 'matern5', 22),
}
OTHER = {'se': 'matern5', 'matern5': 'se'}


def second_objective(X, seed):
    return np.cos(2.0 * X.sum(1)) + 0.3 * np.sin(4.0 * X[:, 1]) + 1e-2 * np.random.RandomState(seed + 7).randn(len(X))


def build(N, d, kernel, seed, m=M):
    """dict(X, Y (N, 2), Z (m, d), kernels (2), hypers [(sn2, rho, ell (d,), bias)] x 2)."""
    X, y, ell = synth_problem(N, d, seed=seed)
    Y = np.column_stack([y, second_objective(X, seed)])
    Z = np.random.RandomState(seed + 100).rand(m, d)
    hypers = [(sn2, rho, ell * f, bias) for sn2, rho, f, bias in HYPERS[:2]]
    return dict(N=N, d=d, seed=seed, X=X, Y=Y, Z=Z, kernels=(kernel, OTHER[kernel]), hypers=hypers)


def problem(name, m=M):
    return build(*CASES[name], m=m)


def raw_front(n, seed, lo=-1.0, hi=1.0):
    """(P, ref): a raw point set of which exactly n points form the front over ref -- a staircase between lo and hi in both objectives --
    together with exact duplicates, dominated points, points below ref and points on its edges, shuffled."""
    rng = np.random.RandomState(seed)
    t = (np.arange(1, n + 1) - 0.5) / n
    front = np.column_stack([lo + (hi - lo) * t, hi - (hi - lo) * t])
    ref = np.array([lo - 0.5, lo - 0.5])
    step = (hi - lo) / n
    pick = rng.randint(0, n, size=2 * n + 5)
    how = rng.randint(0, 4, size=len(pick))
    extra = front[pick].copy()
    extra[how == 1] -= 0.25 * step * (1.0 + rng.rand((how == 1).sum(), 2))      # dominated by the point it came from
    extra[how == 2, 0] = ref[0]                                                 # on the reference point's edge
    extra[how == 3] = ref - rng.rand((how == 3).sum(), 2)                       # below it
    P = np.vstack([front, extra])
    return P[rng.permutation(len(P))], ref


def synthetic_moments(m, seed, lo=-1.0, hi=1.0):
    """(4, m): mu1, s2_1, mu2, s2_2 that put the front's thresholds anywhere between z = -40 and z = +40 on both objectives, with
    variances from the floor of the device's s2 (1e-100) up to 25; entry 0 of mu1 is NaN and entry 1 of mu2 +inf where m allows."""
    rng = np.random.RandomState(seed)
    mom = np.empty((4, m))
    for j in (0, 1):
        s2 = np.exp(rng.uniform(np.log(1e-6), np.log(25.0), size=m))
        s2[rng.rand(m) < 0.1] = 1e-100
        centre = rng.uniform(lo - 0.5, hi, size=m)
        z = rng.uniform(-40.0, 40.0, size=m)
        mom[2 * j] = centre + z * np.sqrt(s2)
        mom[2 * j + 1] = s2
    if m > 2:
        mom[0, 0] = np.nan
        mom[2, 1] = np.inf
    return mom
