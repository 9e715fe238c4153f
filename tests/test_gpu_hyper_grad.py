"""gpx_loglik_grad on the device against the numpy gradient of tests/hyper_ref.py: within 1e-6 S per component, S the
cancellation-free scale of each sum (the project's tolerance for derived quantities).  Unless stated
otherwise sn2 = 1e-2 rho (conditioning ~1e4: the reference itself is well inside the tolerance)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hyper_ref                                            # noqa: E402
from oracle import gp_ref                                   # noqa: E402
from pybo_amd import _lib, models                           # noqa: E402

opt = importlib.import_module('pybo_amd.models.optimize')

pytestmark = pytest.mark.gpu
TOL = 1e-6
WORST = [0.0]


def make_data(N, d, seed=0, dup=0):
    rng = np.random.RandomState(1000 * seed + 7 * N + d)
    X = rng.rand(N, d)
    for i in range(dup):                                    # duplicated rows
        X[(3 * i + 5) % N] = X[(7 * i + 1) % N]
    y = np.sin(3.0 * X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(N)
    ell = (0.2 + 0.3 * rng.rand(d)) * np.sqrt(d)
    return X, y, ell


def oracle(X, y, kernel, ell, rho, sn2, bias):
    ref = gp_ref.GPRef(sn2, rho, ell, bias, kernel)
    ref.add_data(X, y)
    grad, S = hyper_ref.loglik_grad(ref)
    return ref, grad, S


def check(eng, X, y, kernel, ell, rho, sn2, bias, what):
    ref, want, S = oracle(X, y, kernel, ell, rho, sn2, bias)
    L, g = eng.loglik_grad()
    assert L == eng.loglik()                                # bit for bit gpx_loglik's value
    assert abs(L - ref.loglikelihood()) <= 1e-9 * max(1.0, abs(ref.loglikelihood()))
    err = np.abs(g - want)
    rel = np.divide(err, S, out=np.zeros_like(err), where=S > 0)        # S = 0 (N = 1: no pair for a length-scale): err must be 0
    WORST[0] = max(WORST[0], float(rel.max()))
    print('%s: max |dev - ref| / S = %.3g (component %d); largest so far %.3g' % (what, rel.max(), rel.argmax(), WORST[0]))
    assert np.all(err <= TOL * S), (what, err, S)
    return L, g


@pytest.fixture(scope='module')
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize('d', [1, 8, 33])
@pytest.mark.parametrize('N', [1, 127, 128, 129, 300, 700])
def test_parity_over_the_tilings(eng, N, d):
    """One block, a padded block, an exact block, a 1-row spill, 3 and 6 block rows (700: the task-graph factorisation and the
    Tile128 levels of the inverse); d = 33 crosses the 32-coordinate slab.  Largest |dev - ref| / S observed over this file:
    not recorded yet (no GPU run so far); every case prints its figure and the running maximum (-s)."""
    X, y, ell = make_data(N, d)
    rho = 1.3
    eng.fit(X, y, 'se', ell, rho, 1e-2 * rho, 0.0)
    check(eng, X, y, 'se', ell, rho, 1e-2 * rho, 0.0, 'N=%d d=%d' % (N, d))


@pytest.mark.parametrize('kernel', ['se', 'matern5', 'matern3', 'matern1'])
def test_parity_all_kernels(eng, kernel):
    X, y, ell = make_data(300, 8, seed=1)
    rho = 0.7
    eng.fit(X, y, kernel, ell, rho, 1e-2 * rho, 0.0)
    check(eng, X, y, kernel, ell, rho, 1e-2 * rho, 0.0, kernel)


def test_parity_duplicated_rows_matern12(eng):
    X, y, ell = make_data(300, 8, seed=2, dup=6)
    rho = 1.0
    eng.fit(X, y, 'matern1', ell, rho, 1e-2 * rho, 0.0)
    _, g = check(eng, X, y, 'matern1', ell, rho, 1e-2 * rho, 0.0, 'matern1 with duplicated rows')
    assert np.all(np.isfinite(g))


def test_parity_with_a_bias(eng):
    X, y, ell = make_data(300, 8, seed=3)
    rho = 1.0
    eng.fit(X, y + 2.5, 'matern5', ell, rho, 1e-2 * rho, 2.1)
    check(eng, X, y + 2.5, 'matern5', ell, rho, 1e-2 * rho, 2.1, 'bias = 2.1')


def test_two_calls_and_two_handles_give_the_same_bits(eng):
    X, y, ell = make_data(700, 8, seed=4)
    eng.fit(X, y, 'matern3', ell, 1.0, 1e-2, 0.1)
    L1, g1 = eng.loglik_grad()
    L2, g2 = eng.loglik_grad()
    other = _lib.Engine(0)
    try:
        other.fit(X, y, 'matern3', ell, 1.0, 1e-2, 0.1)
        L3, g3 = other.loglik_grad()
    finally:
        other.close()
    assert L1 == L2 == L3
    assert g1.tobytes() == g2.tobytes() == g3.tobytes()


def test_after_append_across_a_block_boundary():
    """Fit at N = 255, append two points: the second one crosses the block boundary and grows the factor."""
    X, y, ell = make_data(257, 3, seed=5)
    e = _lib.Engine(0)
    try:
        e.fit(X[:255], y[:255], 'se', ell, 1.0, 1e-2, 0.0)
        assert e.append(X[255], y[255]) and e.append(X[256], y[256])
        check(e, X, y, 'se', ell, 1.0, 1e-2, 0.0, 'after two appends (N = 257)')
    finally:
        e.close()


def test_leaves_a_live_sweep_cache_alone():
    X, y, ell = make_data(300, 3, seed=6)
    Z = np.random.RandomState(9).rand(4096, 3)
    e = _lib.Engine(0)
    try:
        e.fit(X, y, 'se', ell, 1.0, 1e-2, 0.0)
        e.set_option('sweep_cache', 1)
        e.sweep('ei', float(y.max()), Z, k=8)
        e.set_option('sweep_cache', 0)
        assert e.sweep_cache_size() == len(Z)
        before = e.sweep_update('ei', float(y.max()), k=8)
        e.loglik_grad()
        assert e.sweep_cache_size() == len(Z)
        after = e.sweep_update('ei', float(y.max()), k=8)
        for key in ('top_val', 'top_idx', 'acq'):
            assert before[key].tobytes() == after[key].tobytes(), key
    finally:
        e.close()


def test_errors_leave_the_handle_usable():
    lib = _lib.load()
    e = _lib.Engine(0)
    try:
        g = np.empty(8)
        L = C.c_double()
        assert lib.gpx_loglik_grad(e._h, C.byref(L), _lib._ptr(g)) == _lib.GPX_ESTATE        # before any fit
        X, y, ell = make_data(129, 2, seed=7)
        e.fit(X, y, 'se', ell, 1.0, 1e-2, 0.0)
        assert lib.gpx_loglik_grad(e._h, C.byref(L), None) == _lib.GPX_EARG                  # NULL grad
        assert lib.gpx_loglik_grad(e._h, None, _lib._ptr(g)) == _lib.GPX_OK                   # loglik may be NULL
        check(e, X, y, 'se', ell, 1.0, 1e-2, 0.0, 'after the refused calls')
    finally:
        e.close()


def test_python_layer_applies_the_chain_rule():
    X, y, ell = make_data(300, 4, seed=8)
    gp = models.make_gp(2e-2, 1.7, ell, 0.2, kernel='matern5')
    gp.add_data(X, y)
    L, g = gp.loglikelihood(grad=True)
    Le, ge = gp._engine().loglik_grad()
    assert L == Le == gp.loglikelihood()
    np.testing.assert_array_equal(g, ge * np.concatenate([[2e-2, 1.7], ell, [1.0]]))
    ref, want, S = oracle(X, y, 'matern5', ell, 1.7, 2e-2, 0.2)
    assert np.all(np.abs(g - hyper_ref.to_theta(ref, want)) <= TOL * hyper_ref.to_theta(ref, S))


def test_optimize_reaches_the_oracle_optimum():
    """The CPU test's problem (hyper_ref.opt_problem, start truth + 0.5): the device model's MAP state, scored by the ORACLE's
    target, is no worse than the start and within 1e-6 max(1, |target|) of the optimum GPRefGrad reaches."""
    X, y, truth, bounds = hyper_ref.opt_problem()
    d = X.shape[1]
    th0 = truth + 0.5

    def fresh(cls, **kw):
        m = cls(np.exp(th0[0]), np.exp(th0[1]), np.exp(th0[2:2 + d]), th0[2 + d], **kw)
        hyper_ref.init_model_priors(m, y, bounds)
        m.add_data(X, y)
        return m
    ref = opt.optimize(fresh(hyper_ref.GPRefGrad, kernel='se'))
    best = opt.log_target_grad(ref, ref.hyper_vector())[0]
    gp = fresh(models.GP, kernel='se')
    assert gp.optimize() is gp
    judge = fresh(hyper_ref.GPRefGrad, kernel='se')
    start = opt.log_target_grad(judge, th0)[0]
    got = opt.log_target_grad(judge, gp.hyper_vector())[0]
    print('oracle target: start %.6f, device optimum %.9f, oracle optimum %.9f' % (start, got, best))
    assert got >= start
    assert abs(got - best) <= 1e-6 * max(1.0, abs(best))
