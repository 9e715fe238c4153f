"""The long-double restatement of the selection-only sweep's bound (oracle/gp_ref.py: prune_truth, prune_delta,
sel_key24), checked without a GPU: on a numpy fp64 emulation of both means -- the bound pass's row-dot and the exact
chain's V^T a in three summation orders -- for one well- and one ill-conditioned model, |mean - mu_true| stays inside
delta / 2 (delta is twice the first-order total), S in fp64 agrees with the long-double S to
(Np + 8) u, and EI(mu_est + delta, sqrt(rho)) bounds EI(mu_true, sqrt(rho)).  The margins are printed (-s): what plain
fp64 summation leaves of delta before the device is asked (tests/test_gpu_prune_bound.py)."""
import numpy as np
import pytest
import scipy.linalg as sla

import bench
import devmath_ref
from oracle import gp_ref
from helpers import synth_problem


def _model(which):
    if which == 'well':
        N, d = 700, 5
        X, y, ell = synth_problem(N, d, seed=3)
        rho, sn2, bias, kern = 1.3, 1e-3, 0.2, 'matern5'
        Z = np.random.RandomState(5).rand(300, d)
    else:                                   # config B's inputs at the reference's literal default noise
        w = bench.make_workload('b', 256)
        X, y, ell, rho, bias, kern = w['X'], w['y'], w['ell'], w['rho'], w['bias'], 'se'
        sn2 = 1e-6
        Z = w['Xc']
    K = gp_ref.kernel(gp_ref.KERNEL_IDS[kern], X, X, ell, rho)
    K[np.diag_indices_from(K)] += sn2
    L = np.linalg.cholesky(K)
    T = sla.solve_triangular(L, np.eye(len(L)), lower=True)
    a = T @ (y - bias)
    Ks = gp_ref.kernel(gp_ref.KERNEL_IDS[kern], X, Z, ell, rho)
    return T, a, Ks, rho, bias


@pytest.mark.parametrize('which', ['well', 'ill'])
def test_fp64_means_stay_inside_half_delta_of_the_long_double_mean(which):
    T, a, Ks, rho, bias = _model(which)
    N = len(a)
    Np = (N + 127) // 128 * 128
    mu_true, S = gp_ref.prune_truth(T, a, Ks, rho, bias)
    S64 = float(np.sum(np.abs(T).T @ np.abs(a)))
    assert abs(S64 - float(S)) <= (Np + 8) * gp_ref.U53 * float(S)
    delta = gp_ref.prune_delta(S64, Np, rho, bias)
    assert delta == 8.0 * (Np + 16) * 2.0 ** -53 * devmath_ref.fma(rho, S64, abs(bias))
    # the long-double mean is the exact-GP mean (the oracle's substitution), far inside delta where the model is benign
    worst = {}
    for name, mu in gp_ref.prune_mean_emulations(T, a, Ks, bias).items():
        err = np.abs(mu.astype(np.longdouble) - mu_true).astype(float)
        worst[name] = err.max() / delta
        assert np.all(err <= delta / 2), name
    print('\n%s: N = %d, S = %.3e, delta = %.3e, max |mu - mu_true| / delta: %s'
          % (which, N, S64, delta, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    # the bound itself: EI(mu_est + delta, sqrt(rho)) >= EI(mu_true, sqrt(rho)), both at 50 digits
    est = gp_ref.prune_mean_emulations(T, a, Ks, bias)['rowdot']
    target = float(np.max(mu_true))
    for n in np.linspace(0, len(est) - 1, 16).astype(int):
        ub = devmath_ref.acq_truth('ei', est[n] + delta, rho, target)
        assert ub >= devmath_ref.acq_truth('ei', float(mu_true[n]), rho, target)


def test_sel_key24_is_monotone_and_keeps_twelve_mantissa_bits():
    v = np.array([-np.inf, -1e300, -1.0, -1e-300, -0.0, 0.0, 5e-324, 1e-300, 1.0, 1.0 + 2.0 ** -12, 2.0, 1e300, np.inf, np.nan])
    k = gp_ref.sel_key24(v)
    assert np.all(np.diff(k) >= 0) and k.min() >= 0 and k.max() < 1 << 24
    assert k[-1] == k.max() and k[-1] > k[-2]                      # a (positive) NaN sorts above +inf
    assert gp_ref.sel_key24([1.0 + 2.0 ** -13])[0] == gp_ref.sel_key24([1.0])[0] != gp_ref.sel_key24([1.0 + 2.0 ** -12])[0]
    r = np.random.RandomState(0).randn(10000) * 10.0 ** np.random.RandomState(1).randint(-300, 300, 10000)
    o = np.argsort(r)
    assert np.all(np.diff(gp_ref.sel_key24(r[o])) >= 0)
