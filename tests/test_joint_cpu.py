"""Host side of the joint posterior (no device): the prior of a model without data, empty inputs, the point limit, the ensemble's
mixture draws, and the header / binding-table agreement for the two new entry points."""
import os
import re

import numpy as np
import pytest

from oracle import gp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('se', 'matern5', 'matern3', 'matern1')


@pytest.mark.parametrize('kernel', KERNELS)
def test_a_model_without_data_returns_its_prior(kernel):
    from pybo_amd import models
    rho, bias, ell = 1.7, 0.4, np.array([0.3, 0.5, 0.2])
    gp = models.make_gp(1e-3, rho, ell, bias, kernel=kernel)
    X = np.random.RandomState(1).rand(37, 3)
    mu, cov = gp.predict_cov(X)
    K = gp_ref.kernel(gp_ref.KERNEL_IDS[kernel], X, X, ell, rho)
    assert mu.shape == (37,) and np.all(mu == bias)
    assert cov.shape == (37, 37) and np.abs(cov - K).max() <= 1e-14 * rho
    one, three = gp.sample(X, rng=3), gp.sample(X, size=3, rng=3)
    assert one.shape == (37,) and three.shape == (3, 37)
    assert np.array_equal(three, gp.sample(X, size=3, rng=3)) and np.array_equal(one, gp.sample(X, rng=3))
    np.testing.assert_allclose(one, three[0], rtol=0, atol=1e-12 * np.sqrt(rho))            # the same stream of normals
    # the host factor carries the same jitter: the draws are bias + z R with R^T R = K + 1e-10 rho I
    z = np.random.RandomState(3).randn(3, 37)
    L = np.linalg.cholesky(K + 1e-10 * rho * np.eye(37))
    np.testing.assert_allclose(three, bias + z @ L.T, rtol=0, atol=1e-9 * np.sqrt(rho))
    noisy = gp.sample(X, size=3, latent=False, rng=3)
    assert noisy.shape == (3, 37) and not np.array_equal(noisy, three)


def test_empty_input_and_the_point_limit_need_no_device():
    from pybo_amd import models
    gp = models.make_gp(1e-3, 1.0, [0.3, 0.3], 0.1)
    gp._X, gp._Y = np.random.rand(5, 2), np.random.rand(5)          # data, but never fitted: any device call would raise here
    mu, cov = gp.predict_cov(np.zeros((0, 2)))
    assert mu.shape == (0,) and cov.shape == (0, 0)
    assert gp.sample(np.zeros((0, 2))).shape == (0,)
    assert gp.sample(np.zeros((0, 2)), size=3).shape == (3, 0)
    big = np.zeros((4097, 2))
    for call in (lambda: gp.predict_cov(big), lambda: gp.sample(big), lambda: gp.sample(big, size=2, latent=False)):
        with pytest.raises(ValueError, match='4096'):
            call()
    with pytest.raises(ValueError):
        gp.sample(np.zeros((3, 2)), jitter=-1.0)
    sh = models.make_gp(1e-3, 1.0, [0.3, 0.3], 0.1, devices=[0])
    assert sh.predict_cov(np.zeros((0, 2)))[1].shape == (0, 0) and sh.sample(np.zeros((0, 2)), size=2).shape == (2, 0)
    with pytest.raises(ValueError, match='4096'):
        sh.sample(big)
    assert not hasattr(models.MCMC, 'predict_cov')                 # no ensemble covariance


class _Member(object):
    """A stand-in member: its draws are its own index, and it consumes the shared stream as a GP does (M normals per draw)."""

    def __init__(self, k, log):
        self.k, self.log = k, log

    def sample(self, X, size=None, latent=True, rng=None, jitter=None):
        assert size is None
        self.log.append((self.k, latent, jitter))
        return self.k + 0.0 * rng.randn(len(X))


def test_the_ensemble_draws_each_sample_from_a_member_chosen_by_rng():
    from pybo_amd.models import MCMC
    from pybo_amd.utils import rstate
    log = []
    ens = MCMC.__new__(MCMC)
    ens._members = [_Member(k, log) for k in range(5)]
    X = np.zeros((7, 2))
    out = ens.sample(X, size=6, latent=False, rng=11, jitter=1e-9)
    assert out.shape == (6, 7)
    # the picks are the stream's: randint, then the member's M normals, per draw
    rng = rstate(11)
    want = []
    for _ in range(6):
        want.append(rng.randint(5))
        rng.randn(7)
    assert [int(r[0]) for r in out] == want and all(np.all(r == r[0]) for r in out)
    assert log == [(k, False, 1e-9) for k in want]
    assert len(set(want)) > 1
    assert np.array_equal(out, ens.sample(X, size=6, latent=False, rng=11, jitter=1e-9))
    assert ens.sample(X, rng=11).shape == (7,) and ens.sample(X, size=0, rng=11).shape == (0, 7)


def test_header_and_binding_table_declare_the_joint_entry_points():
    from pybo_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gpx.h')).read(), flags=re.S)
    names = sorted(set(re.findall(r'\b(gpx_[a-z_0-9]+)\s*\(', src)))
    assert names == sorted(_lib.SYMBOLS)
    assert 'gpx_predict_cov' in names and 'gpx_sample_joint' in names
    assert len(_lib.SYMBOLS['gpx_predict_cov'][1]) == 5 and len(_lib.SYMBOLS['gpx_sample_joint'][1]) == 8
    assert _lib.TIMER_NAMES[21] == 'joint' and len(_lib.TIMER_NAMES) == 22
    lib = _lib.load()
    assert hasattr(lib, 'gpx_predict_cov') and hasattr(lib, 'gpx_sample_joint')
