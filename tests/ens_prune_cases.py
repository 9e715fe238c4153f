"""The small ensemble problems shared by test_ens_prune_cpu.py (the oracle's survivor count) and test_gpu_ens_prune.py
(DESIGN.md section 2.2).  Smallest shapes at which the selection-only ensemble sweep can still go wrong: N = 300 is three
block rows, so a generation is G = 4096 candidates and pruning is legal from M = 3 G = 12288; M = 13001 is off the tile
grid; N = 1100 (+ 2 appended observations; N = 1151 + 2 crosses a block row) is nine / ten block rows, G still 4096.
Sparse data (d = 6 .. 8): the prior variance bounds EI well there, so the oracle's survivors stay inside the cap
(test_ens_prune_cpu.py asserts it) and "path == pruned" on the device is a statement about the code, not the inputs."""
import numpy as np

from helpers import synth_problem

# (sn2, rho, factor on the problem's length scales, bias) of up to four members, all distinct
HYPERS = [(1e-3, 1.0, 1.00, 0.0), (5e-3, 1.6, 1.30, 0.2), (2e-4, 0.7, 0.80, -0.1), (1e-2, 1.2, 1.60, 0.05)]
KS = (1, 10, 200)
G = 4096                      # one generation for up to 31 block rows and k <= 4096
M = 13001

# name -> N at the fit, appended observations, d, kernel, members.  Every one is meant to prune at every k of KS.
CASES = {
    'se_n3': dict(N=300, app=0, d=8, kernel='se', n=3, seed=14),
    'se_n1': dict(N=300, app=0, d=7, kernel='se', n=1, seed=13),
    'm5_n4': dict(N=300, app=0, d=6, kernel='matern5', n=4, seed=12),
    'm5_n3_d5': dict(N=300, app=0, d=5, kernel='matern5', n=3, seed=16),      # the one whose survivor list is not empty (k = 200)
    'se_n3_app': dict(N=1100, app=2, d=8, kernel='se', n=3, seed=15),
    'm5_n3_cross': dict(N=1151, app=2, d=8, kernel='matern5', n=3, seed=11),
}


def cap_of(m):
    return max(G, m // 4)


def problem(name, m=M):
    """dict(X, y (the N + app observations, the last `app` to be appended), Z (m, d), hypers [(sn2, rho, ell (d,), bias)], target)."""
    c = CASES[name]
    seed = c['seed']
    X, y, ell = synth_problem(c['N'] + c['app'], c['d'], seed=seed)
    Z = np.random.RandomState(seed + 100).rand(m, c['d'])
    hypers = [(sn2, rho, ell * f, bias) for sn2, rho, f, bias in HYPERS[:c['n']]]
    return dict(c, X=X, y=y, Z=Z, hypers=hypers, target=float(np.max(y)))


def ei(mu, s, target):
    """Expected improvement over `target` of N(mu, s^2) (oracle/gp_ref.py GPRef.get_improvement's formula)."""
    from oracle import gp_ref
    z = (mu - target) / s
    return (mu - target) * gp_ref.norm_cdf(z) + s * gp_ref.norm_pdf(z)


def ens_mean(rows):
    """Member-order float64 sum, one division by n: the association of the device's accumulate and finish kernels."""
    acc = np.array(rows[0], dtype=np.float64, copy=True)
    for r in rows[1:]:
        acc = acc + r
    return acc / float(len(rows))


def survivors(ub, value_of, k, done=0):
    """The selection of DESIGN.md 2.1 / 2.2 restated: seeds = the G largest bounds among the candidates from `done` on (ties: the
    first by index), tau = the k-th best value among the seeds, survivors = the others whose bound is not below
    tau (1 - 1e-6) (all of them where tau < 1e-280).  value_of(idx) -> exact values.  Returns (seed idx, tau, survivor idx)."""
    b = np.array(ub, dtype=np.float64, copy=True)
    b[:done] = -np.inf
    key = np.where(np.isnan(b), np.inf, b)
    seeds = np.sort(np.lexsort((np.arange(len(b)), -key))[:G])
    v = value_of(seeds)
    v = np.sort(np.where(np.isnan(v), -np.inf, v))[::-1]
    tau = v[k - 1]
    b[seeds] = -np.inf
    cut = tau * (1.0 - 1e-6) if tau >= 1e-280 else -np.inf
    return seeds, tau, np.flatnonzero(~(b < cut))
