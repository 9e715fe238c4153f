"""CPU checks of the hyper-parameter gradient: the numpy formula (tests/hyper_ref.py) against central differences of the
oracle's evidence, the prior gradients, `pybo_amd.models.optimize` on the oracle model, and the new entry point's
export.  Tolerances are relative to the cancellation-free scales S of hyper_ref, never to the gradient."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hyper_ref                                            # noqa: E402
from oracle import gp_ref                                   # noqa: E402
opt = importlib.import_module('pybo_amd.models.optimize')   # the module (pybo_amd.models.optimize is its function)
from pybo_amd.models import priors                          # noqa: E402

KERNELS = ('se', 'matern5', 'matern3', 'matern1')


def make_case(kernel, N, d, seed=0, dup=True, bias=0.3, rho=1.3, sn2=1e-2, cls=gp_ref.GPRef):
    rng = np.random.RandomState(seed + 7 * N + d)
    X = rng.rand(N, d)
    if dup:
        X[N // 2] = X[3]                                    # one duplicated row (Matern-1/2: g = 0 at r2 = 0)
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.randn(N) + bias
    gp = cls(sn2, rho, 0.2 + 0.3 * rng.rand(d), bias, kernel)
    gp.add_data(X, y)
    return gp


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('N,d', [(130, 3), (300, 5)])
def test_formula_agrees_with_central_differences(kernel, N, d):
    """Measured on the CPU: <= 1.2e-9 S in every component (Matern-1/2 included); asserted at 1e-7 S."""
    gp = make_case(kernel, N, d)
    grad, S = hyper_ref.loglik_grad(gp)
    g_th, S_th = hyper_ref.to_theta(gp, grad), hyper_ref.to_theta(gp, S)
    th0, h = gp.hyper_vector(), 1e-5
    fd = np.empty(d + 3)
    for c in range(d + 3):
        e = np.zeros(d + 3)
        e[c] = h
        gp.set_hyper_vector(th0 + e)
        up = gp.loglikelihood()
        gp.set_hyper_vector(th0 - e)
        fd[c] = (up - gp.loglikelihood()) / (2 * h)
    rel = np.abs(g_th - fd) / S_th
    print('%s N=%d d=%d  max |analytic - FD| / S = %.3g' % (kernel, N, d, rel.max()))
    assert np.all(rel <= 1e-7), rel


@pytest.mark.parametrize('prior,xs', [
    (('horseshoe', 0.1), [1e-3, 0.05, 0.7, 4.0]),
    (('lognormal', np.log(1.3), 1.0), [1e-2, 0.4, 1.3, 9.0]),
    (('normal', 0.2, 1.7), [-3.0, 0.0, 0.2, 2.5]),
    (('uniform', 0.01, 3.0), [0.02, 0.5, 2.9]),
])
def test_prior_gradients_agree_with_central_differences(prior, xs):
    for x in xs:
        h = 1e-6 * max(1.0, abs(x))
        fd = (priors.log_prior(prior, x + h) - priors.log_prior(prior, x - h)) / (2 * h)
        g = float(priors.log_prior_grad(prior, x))
        assert abs(g - fd) <= 1e-6 * max(1.0, abs(fd)), (prior[0], x, g, fd)
        if prior[0] == 'uniform':
            assert g == 0.0
    v = np.array(xs)                                        # vectors: element-wise
    np.testing.assert_allclose(priors.log_prior_grad(prior, v), [float(priors.log_prior_grad(prior, x)) for x in xs])
    assert np.all(priors.log_prior_grad(None, v) == 0.0)
    lo, hi = priors.prior_bounds(prior, 2)
    if prior[0] == 'uniform':
        assert np.all(lo == 0.01) and np.all(hi == 3.0)
    else:
        assert np.all(np.isinf(lo)) and np.all(np.isinf(hi))


def opt_model(start_shift, cls=hyper_ref.GPRefGrad):
    X, y, truth, bounds = hyper_ref.opt_problem()
    d = X.shape[1]
    th = truth + start_shift
    gp = cls(np.exp(th[0]), np.exp(th[1]), np.exp(th[2:2 + d]), th[2 + d], 'se')
    hyper_ref.init_model_priors(gp, y, bounds)
    gp.add_data(X, y)
    return gp


def test_target_gradient_agrees_with_central_differences():
    """The whole target (likelihood + priors + Jacobian) in theta, as optimize() hands it to L-BFGS-B."""
    gp = opt_model(0.5)
    th0 = gp.hyper_vector()
    f0, g = opt.log_target_grad(gp, th0)
    for c in range(len(th0)):
        e = np.zeros(len(th0))
        e[c] = 1e-5
        fd = (opt.log_target_grad(gp, th0 + e)[0] - opt.log_target_grad(gp, th0 - e)[0]) / 2e-5
        assert abs(g[c] - fd) <= 1e-6 * max(1.0, abs(fd)), (c, g[c], fd)


def test_optimize_on_the_oracle_model():
    """Seed hyper_ref.OPT_SEED = 17 (chosen on the CPU, see there): from truth + 0.5 the projected gradient ends at 1.8e-6 <= pgtol,
    and the start truth + 0.45 ends in the same optimum (targets 4e-10 apart)."""
    pgtol = 1e-5
    gp, info = opt_model(0.5), {}
    start = opt.log_target_grad(gp, gp.hyper_vector())[0]
    assert opt.optimize(gp, maxiter=200, pgtol=pgtol, info=info) is gp
    th = info['theta']
    np.testing.assert_allclose(gp.hyper_vector(), th, rtol=0, atol=1e-14)       # (exp / log round trip)
    f, g = opt.log_target_grad(gp, th)
    assert f == info['target'] and f >= start == info['start_target']          # the target did not decrease
    lo, hi = info['bounds']
    proj = np.clip(th + g, lo, hi) - th                     # projected gradient of the MAXIMISATION over the box
    print('target %.6f -> %.6f in %d evaluations, |projected gradient|_inf = %.3g' % (start, f, info['nfev'], np.abs(proj).max()))
    assert np.abs(proj).max() <= pgtol
    gp2 = opt.optimize(opt_model(0.45), maxiter=200, pgtol=pgtol)
    f2 = opt.log_target_grad(gp2, gp2.hyper_vector())[0]
    assert abs(f2 - f) <= 1e-6 * max(1.0, abs(f)), (f, f2)
    np.testing.assert_allclose(gp2.hyper_vector(), th, atol=1e-3)


def test_optimize_backs_off_from_states_without_a_density():
    """A refused proposal (LinAlgError / -inf) costs a large finite value: the search ends at a finite state no worse than the start."""
    class Picky(hyper_ref.GPRefGrad):
        def loglikelihood(self, grad=False):
            if self.ell[0] > 0.3:
                raise np.linalg.LinAlgError('refused')
            return hyper_ref.GPRefGrad.loglikelihood(self, grad)
    gp, info = opt_model(0.0, cls=Picky), {}
    opt.optimize(gp, maxiter=50, info=info)
    assert np.isfinite(info['target']) and info['target'] >= info['start_target'] and gp.ell[0] <= 0.3


def test_symbol_is_exported_and_bound():
    from pybo_amd import _lib
    lib = _lib.load()
    assert 'gpx_loglik_grad' in _lib.SYMBOLS and hasattr(lib, 'gpx_loglik_grad')
    assert hasattr(_lib.Engine, 'loglik_grad')
