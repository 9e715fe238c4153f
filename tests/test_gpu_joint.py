"""gpx_predict_cov / gpx_sample_joint on the device against the CPU oracle (tests/joint_ref.py): the full covariance
Sigma = k(Z, Z) - V^T V, its bit-for-bit symmetry and determinism, the factor R^T R = Sigma + c I behind the draws, the draws
themselves, what the calls leave alone (fit, sweep cache, a pending announcement), the refused arguments, and the plug-in
methods GP.predict_cov / GP.sample / ShardedGP.  Tolerances: DESIGN.md section 6 (mean, variance -- carried to off-diagonal
entries by Cauchy-Schwarz -- and the factorisation's 1e-13)."""
import numpy as np
import pytest

import joint_ref
from joint_ref import RHO, BIAS, SN2
from helpers import mu_tol

pytestmark = pytest.mark.gpu

JIT = 1e-10 * RHO
EPS = 2.0 ** -52


def _engine(c):
    """A handle fitted on the case's observations (the appended ones left out), then extended by gpx_append."""
    from pybo_amd._lib import Engine
    n0 = len(c['X']) - c['nappend']
    e = Engine(0)
    e.fit(c['X'][:n0], c['y'][:n0], c['kernel'], c['ell'], RHO, SN2, BIAS)
    for i in range(n0, len(c['X'])):
        assert e.append(c['X'][i], c['y'][i])
    return e


def _factor(e, Z, mu, noisy):
    """R of the device's factorisation through the draws of z = I: D = out - mu."""
    M = len(Z)
    return e.sample_joint(Z, np.eye(M), noisy=noisy, jitter=JIT) - mu[None, :]


@pytest.mark.parametrize('tag', sorted(joint_ref.CASES))
def test_joint_posterior_matches_the_oracle(tag):
    c = joint_ref.case(tag)
    Z, M = c['Z'], len(c['Z'])
    e = _engine(c)
    mu, cov = e.predict_cov(Z)
    tol = joint_ref.cov_tol(c['Sigma'])
    print(tag, 'mu err/tol %.3g  cov err/tol %.3g' % ((np.abs(mu - c['mu']) / mu_tol(c['mu'], RHO)).max(),
                                                        (np.abs(cov - c['Sigma']) / tol).max()))
    # 1. mean  2. covariance, and its diagonal against gpx_predict on the same handle  3. symmetry, bit for bit
    assert np.all(np.abs(mu - c['mu']) <= mu_tol(c['mu'], RHO))
    assert np.all(np.abs(cov - c['Sigma']) <= tol)
    s2 = e.predict(Z)[1]
    assert np.all(np.abs(np.diag(cov) - s2) <= np.diag(tol))
    assert np.array_equal(cov, cov.T)
    # 4. determinism: the same bits again, also with mu left out
    mu2, cov2 = e.predict_cov(Z)
    assert np.array_equal(mu, mu2) and np.array_equal(cov, cov2)
    # 6. the factor: upper triangular, R^T R = Sigma_dev + c I to the factorisation's tolerance
    R = None
    for noisy in (False, True):
        D = _factor(e, Z, mu, noisy)
        assert np.array_equal(D, np.triu(D))
        A = cov + (JIT + (SN2 if noisy else 0.0)) * np.eye(M)
        res = np.linalg.norm(D.T @ D - A) / np.linalg.norm(A)
        print(tag, 'noisy', noisy, 'factor residual %.3g' % res)
        assert res <= 1e-13
        if not noisy:
            R = D
    # 7. draws: against mu_dev + z R_dev with the rounding of an M-term dot product; a draw's bits do not depend on S.
    # R_dev as item 6 recovers it, D = fl(fl(mu + R) - mu), carries eps |mu| of rounding per entry -- with |R| << |mu| that alone
    # is M eps |mu| |z| in z @ D, far above the bound below, and it is the test's error, not the device's.  So the reference's R is
    # read through z = 2^40 I, where mu + 2^40 R rounds relative to R (2 eps |R| per entry; zeros stay exact), and the reference's
    # dot product runs in extended precision: what is left on the right-hand side is the device's own M-term fma chain and add.
    Rx = (e.sample_joint(Z, 2.0 ** 40 * np.eye(M), jitter=JIT) - mu[None, :]) * 2.0 ** -40
    assert np.array_equal(Rx, np.triu(Rx)) and np.all(np.abs(Rx - R) <= 2.0 * EPS * (np.abs(mu)[None, :] + np.abs(R)))
    z = np.random.RandomState(7).randn(3, M)
    out3 = e.sample_joint(Z, z, jitter=JIT)
    out1 = e.sample_joint(Z, z[:1], jitter=JIT)
    want = (mu[None, :].astype(np.longdouble) + z.astype(np.longdouble) @ Rx.astype(np.longdouble))
    bound = (M + 2) * EPS * (np.abs(z) @ np.abs(Rx)) + EPS * np.abs(mu)[None, :]
    print(tag, 'draw err/bound %.3g' % float((np.abs(out3 - want) / bound).max()))
    assert np.all(np.abs(out3 - want) <= bound)
    assert np.array_equal(out3[0], out1[0])
    assert out1.shape == (1, M) and out3.shape == (3, M)
    e.close()


def test_bits_do_not_depend_on_other_work_or_on_the_other_points():
    """After an unrelated full sweep the same bits; the leading 128 x 128 block of the M = 257 matrix IS the M = 128 matrix (a
    tile's contraction runs over all rows of V in one fixed order and reads nothing of the other panels)."""
    c = joint_ref.case('matern5_m257')
    Z = c['Z']
    e = _engine(c)
    mu, cov = e.predict_cov(Z)
    e.sweep('ei', 0.3, np.random.RandomState(3).rand(3000, c['d']), k=5)
    mu_b, cov_b = e.predict_cov(Z)
    assert np.array_equal(mu, mu_b) and np.array_equal(cov, cov_b)
    mu128, cov128 = e.predict_cov(Z[:128])
    assert np.array_equal(cov128, cov[:128, :128]) and np.array_equal(mu128, mu[:128])
    e.close()


def test_sweep_cache_and_a_pending_announcement_are_left_alone():
    """sweep_cache = 1, a full sweep, gpx_append_begin; then both joint calls.  gpx_sweep_update returns the bits it returned
    before them, and the following gpx_append and re-score give the bits of a handle that made no joint call (the announced
    path and the plain one are bit-identical by construction, so the control handle is the witness that nothing was disturbed:
    factor, solve vector and every re-scored output)."""
    c = joint_ref.case('matern5_m257')
    grid = np.random.RandomState(5).rand(4000, c['d'])
    xn, yn = np.array([0.31, 0.62, 0.47]), 0.25
    outs = []
    for with_joint in (True, False):
        e = _engine(c)
        e.set_option('sweep_cache', 1)
        e.sweep('ei', 0.4, grid, k=1, want_all=False)
        e.set_option('sweep_cache', 0)
        before = e.sweep_update('ei', 0.4, k=5, want_moments=True)
        assert e.append_begin(xn)
        if with_joint:
            e.predict_cov(c['Z'])
            e.sample_joint(c['Z'], np.ones((2, len(c['Z']))), noisy=True, jitter=JIT)
            assert e.sweep_cache_size() == len(grid)
        after = e.sweep_update('ei', 0.4, k=5, want_moments=True)
        for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
            np.testing.assert_array_equal(before[key], after[key])
        assert e.append(xn, yn)
        outs.append((e.sweep_update('ei', 0.4, k=5, want_moments=True), e.get_matrix('L'), e.get_vectors()[1]))
        e.close()
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        np.testing.assert_array_equal(outs[0][0][key], outs[1][0][key])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def test_bad_arguments_and_call_order_are_refused():
    from pybo_amd import _lib
    from pybo_amd._lib import Engine, _ptr as P
    c = joint_ref.case('se_m5')
    Z = np.ascontiguousarray(c['Z'])
    big = np.zeros((4097, c['d']))
    z = np.zeros((1, 4097))
    out = np.zeros((1, 4097))
    mu, cov = np.zeros(5), np.zeros((5, 5))
    e = Engine(0)
    lib, h = e._lib, e._h

    def refused(rc, want):
        assert rc == want, rc
        assert len(lib.gpx_last_error(h) or b'') > 0

    # before a fit
    refused(lib.gpx_predict_cov(h, P(Z), 5, P(mu), P(cov)), _lib.GPX_ESTATE)
    refused(lib.gpx_sample_joint(h, P(Z), 5, P(z), 1, 0, 0.0, P(out)), _lib.GPX_ESTATE)
    e.fit(c['X'], c['y'], c['kernel'], c['ell'], RHO, SN2, BIAS)
    s2 = e.predict(Z)[1]
    refused(lib.gpx_predict_cov(h, P(Z), 0, P(mu), P(cov)), _lib.GPX_EARG)
    refused(lib.gpx_predict_cov(h, P(big), 4097, None, P(cov)), _lib.GPX_EARG)
    refused(lib.gpx_predict_cov(h, P(Z), 5, P(mu), None), _lib.GPX_EARG)
    refused(lib.gpx_predict_cov(h, None, 5, P(mu), P(cov)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 0, P(z), 1, 0, 0.0, P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(big), 4097, P(z), 1, 0, 0.0, P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 5, P(z), 1, 0, -1e-12, P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 5, P(z), 1, 0, float('nan'), P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 5, P(z), 1, 0, float('inf'), P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 5, None, 1, 0, 0.0, P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 5, P(z), 0, 0, 0.0, P(out)), _lib.GPX_EARG)
    refused(lib.gpx_sample_joint(h, P(Z), 5, P(z), 1, 0, 0.0, None), _lib.GPX_EARG)
    # mu is optional, and nothing above touched the model
    assert lib.gpx_predict_cov(h, P(Z), 5, None, P(cov)) == _lib.GPX_OK
    np.testing.assert_array_equal(e.predict(Z)[1], s2)
    assert e.fail_pivot() == -1
    e.close()


def test_a_singular_point_set():
    """Two identical rows: Sigma is singular, jitter = 0 leaves the last pivot to rounding (GPX_OK or GPX_ENOTPD, whose text names
    the pivot); either way the model answers as before, gpx_fail_pivot keeps describing the fit, and the default jitter factors."""
    from pybo_amd import _lib
    from pybo_amd._lib import _ptr as P
    c = joint_ref.case('se_m5')
    Z = np.ascontiguousarray(np.vstack([c['Z'], c['Z'][2:3]]))
    M = len(Z)
    e = _engine(c)
    mu, s2 = e.predict(Z)
    z, out = np.ascontiguousarray(np.random.RandomState(1).randn(2, M)), np.zeros((2, M))
    rc = e._lib.gpx_sample_joint(e._h, P(Z), M, P(z), 2, 0, 0.0, P(out))
    assert rc in (_lib.GPX_OK, _lib.GPX_ENOTPD)
    if rc == _lib.GPX_ENOTPD:
        msg = e._lib.gpx_last_error(e._h).decode()
        print(msg)
        assert 'pivot %d' % (M - 1) in msg
    assert e.fail_pivot() == -1
    mu2, s22 = e.predict(Z)
    assert np.array_equal(mu, mu2) and np.array_equal(s2, s22)
    out = e.sample_joint(Z, z, jitter=JIT)
    assert np.all(np.isfinite(out))
    e.close()


def test_plugin_methods():
    from pybo_amd import models
    c = joint_ref.case('matern5_m257')
    Z = c['Z']
    gp = models.make_gp(SN2, RHO, c['ell'], BIAS, kernel=c['kernel'])
    gp.add_data(c['X'], c['y'])
    mu, cov = gp.predict_cov(Z)
    assert np.all(np.abs(mu - c['mu']) <= mu_tol(c['mu'], RHO))
    assert np.all(np.abs(cov - c['Sigma']) <= joint_ref.cov_tol(c['Sigma']))
    a, b = gp.sample(Z, size=4, rng=0), gp.sample(Z, size=4, rng=0)
    assert a.shape == (4, len(Z)) and np.array_equal(a, b)
    np.testing.assert_array_equal(gp.sample(Z, rng=0), a[0])           # one stream of normals, and a draw's bits do not depend on S
    noisy = gp.sample(Z, size=4, latent=False, rng=0)
    assert noisy.shape == a.shape and not np.array_equal(noisy, a)
    sh = models.make_gp(SN2, RHO, c['ell'], BIAS, kernel=c['kernel'], devices=[0])
    sh.add_data(c['X'], c['y'])
    mu_s, cov_s = sh.predict_cov(Z)
    assert np.array_equal(mu_s, mu) and np.array_equal(cov_s, cov)
    assert np.array_equal(sh.sample(Z, size=4, rng=0), a)
    with pytest.raises(ValueError, match='4096'):
        gp.sample(np.zeros((4097, c['d'])))
