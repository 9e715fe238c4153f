"""Pathwise Thompson draws without a GPU: the numpy restatement's own identities (tests/path_ref.py is what tests/test_gpu_path.py holds
the device to), the `method` plumbing of policies.Thompson on a stub, and the binding table."""
import numpy as np
import pytest

import path_ref

CASES = ((300, 3, 100, 5, 1e-4), (129, 20, 130, 3, 1e-6), (1, 2, 100, 2, 1e-2))


def _setup(case, kernel):
    N, d, n, S, snr = case
    m = path_ref.model(N, d, 11 + N, snr, kernel)
    W, b, w = path_ref.spectral(kernel, n, d, m['ell'], S, 5)
    eps = np.random.RandomState(6).randn(S, N)
    sc = np.sqrt(2.0 * m['rho'] / n)
    theta, v, r, Kn = path_ref.weights(kernel, m['X'], m['y'], m['ell'], m['rho'], m['sn2'], m['bias'], W, b, w, eps, sc)
    return m, W, b, w, eps, sc, theta, v, r, Kn


@pytest.mark.parametrize('kernel', ['se', 'matern5', 'matern1'])
@pytest.mark.parametrize('case', CASES)
def test_the_reference_passes_through_the_data_up_to_its_noise(case, kernel):
    """K (K + sn2 I)^-1 = I - sn2 (K + sn2 I)^-1: f_s(X_i) = y_i - sqrt(sn2) eps_si - sn2 v_si.  The reference stays below 1e-4 of the
    tolerance the device is given for the same identity."""
    N, d, n, S, _ = case
    m, W, b, w, eps, sc, theta, v, r, Kn = _setup(case, kernel)
    assert np.array_equal(theta, sc * w)
    f, B = path_ref.values(kernel, m['X'], m['ell'], m['rho'], m['bias'], W, b, theta, v, m['X'])
    want = m['y'][None, :] - np.sqrt(m['sn2']) * eps - m['sn2'] * v
    tol = path_ref.value_tol(B, f, N, n, m['rho']) + path_ref.resid_tol(Kn, v, r)[:, None]
    assert np.all(np.abs(f - want) <= 1e-4 * tol)
    assert np.all(np.linalg.norm(v @ Kn - r, axis=1) <= path_ref.resid_tol(Kn, v, r))


@pytest.mark.parametrize('kernel', path_ref.KERNELS)
def test_without_prior_and_noise_the_reference_is_the_posterior_mean(kernel):
    from oracle import gp_ref
    m = path_ref.model(129, 3, 3, 1e-4, kernel)
    W, b, w = path_ref.spectral(kernel, 100, 3, m['ell'], 2, 5)
    theta, v, r, Kn = path_ref.weights(kernel, m['X'], m['y'], m['ell'], m['rho'], m['sn2'], m['bias'], W, b, 0.0 * w, None, 0.1)
    assert not theta.any() and np.array_equal(r[0], m['y'] - m['bias'])
    Z = np.random.RandomState(1).rand(50, 3)
    f, B = path_ref.values(kernel, m['X'], m['ell'], m['rho'], m['bias'], W, b, theta, v, Z)
    ref = gp_ref.make_gp(m['sn2'], m['rho'], m['ell'], m['bias'], kernel=kernel)
    ref.add_data(m['X'], m['y'])
    mu = ref.predict(Z)[0]
    assert np.all(np.abs(f - mu[None, :]) <= 1e-6 * np.abs(mu) + 1e-9 * np.sqrt(m['rho']))


@pytest.mark.parametrize('kernel', path_ref.KERNELS)
def test_the_reference_gradient_is_the_slope_of_its_value(kernel):
    m = path_ref.model(40, 3, 3, 1e-3, kernel)
    W, b, w = path_ref.spectral(kernel, 30, 3, m['ell'], 1, 5)
    theta, v, _, _ = path_ref.weights(kernel, m['X'], m['y'], m['ell'], m['rho'], m['sn2'], m['bias'], W, b, w, None, 0.2)
    Z = np.random.RandomState(2).rand(6, 3)
    args = (kernel, m['X'], m['ell'], m['rho'], m['bias'], W[0], b[0], theta[0], v[0])
    f, g, Bf, Bg = path_ref.value_grad(*args, Z)
    sw = path_ref.values(kernel, m['X'], m['ell'], m['rho'], m['bias'], W, b, theta, v, Z)[0][0]
    assert np.allclose(f, sw, rtol=1e-12, atol=1e-12) and np.all(Bf >= np.abs(f)) and np.all(Bg >= np.abs(g))
    h = 1e-6
    for j in range(3):
        dz = np.zeros(3)
        dz[j] = h
        num = (path_ref.value_grad(*args, Z + dz)[0] - path_ref.value_grad(*args, Z - dz)[0]) / (2 * h)
        assert np.allclose(g[:, j], num, rtol=1e-5, atol=1e-6 * Bg[:, j].max())
    # on top of an observation the Matern-1/2 kink contributes 0
    if kernel == 'matern1':
        onp = path_ref.value_grad(*args, m['X'][:1])
        assert np.all(np.isfinite(onp[1]))


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def sample_f(self, *args, **kw):
        self.calls.append((args, kw))

        class _S(object):
            @staticmethod
            def get(X, grad=False):
                return np.zeros(len(np.atleast_2d(X)))
        return _S()


def test_thompson_passes_the_method_on_only_when_it_is_asked_for():
    from pybo_amd import policies
    rec = _Recorder()
    index = policies.Thompson(rec, None, None)
    assert rec.calls == [((100, None), {})] and index(np.zeros((3, 2))).shape == (3,)
    policies.Thompson(rec, None, None, n=7, rng=3, method='rff')
    assert rec.calls[-1] == ((7, 3), {})
    policies.Thompson(rec, None, None, n=7, rng=3, method='pathwise')
    assert rec.calls[-1] == ((7, 3), {'method': 'pathwise'})

    class TwoArgs(object):                       # a stub from before the keyword existed
        def sample_f(self, n, rng):
            return _Recorder().sample_f(n, rng)
    assert policies.Thompson(TwoArgs(), None, None, n=5)(np.zeros((2, 1))).shape == (2,)
    # the loop's plumbing accepts the keyword
    from pybo_amd.bayesopt import get_component
    comp = get_component(('thompson', {'method': 'pathwise'}), policies, None)
    comp(rec, None, None)
    assert rec.calls[-1][1] == {'method': 'pathwise'}


def test_the_binding_table_lists_the_new_entry_points():
    from pybo_amd import _lib
    for name in ('gpx_path_weights', 'gpx_path_sweep', 'gpx_path_sweep_dev', 'gpx_path_grad'):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    for name in ('path_weights', 'path_sweep', 'path_sweep_dev', 'path_eval_grad'):
        assert callable(getattr(_lib.Engine, name))
    from pybo_amd.models.gp import GP
    from pybo_amd.models.sharded import ShardedGP
    import inspect
    assert inspect.signature(GP.sample_f).parameters['method'].default == 'rff'
    assert inspect.signature(ShardedGP.sample_f).parameters['method'].default == 'rff'
