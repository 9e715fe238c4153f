"""The truth helpers and bound checkers of tests/devmath_ref.py (used by tests/test_gpu_devmath.py) on the CPU: the truth
agrees with scipy where scipy is accurate, and every checker REJECTS a value that is wrong by a little more than its
bound -- a perturbation of 2 ulp (covariances), 1e-15 absolute (cosines), and the exact numpy emulations of the device's
exp_nonpos and cos_cw with one polynomial term dropped."""
import numpy as np
import mpmath as mp
from scipy import special, stats

import devmath_ref as dm


def test_truth_agrees_with_scipy_at_moderate_arguments():
    r2 = np.linspace(0.01, 30.0, 41)
    for kid, name in enumerate(['se', 'matern5', 'matern3', 'matern1']):
        r = np.sqrt(r2)
        want = {0: np.exp(-0.5 * r2), 1: (1 + np.sqrt(5) * r + 5.0 / 3 * r2) * np.exp(-np.sqrt(5) * r),
                2: (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r), 3: np.exp(-r)}[kid]
        got = np.array([float(dm.kern_truth(kid, x, 1.3)) for x in r2])
        np.testing.assert_allclose(got, 1.3 * want, rtol=1e-14, err_msg=name)
        # dk/dr2 against a central difference of the truth itself
        h = mp.mpf(1e-20)

        def k(v):
            s, poly = dm._kern_s(kid, v)
            return 1.3 * poly * mp.exp(-s)
        for x in r2[::8]:
            fd = (k(mp.mpf(x) + h) - k(mp.mpf(x) - h)) / (2 * h)
            assert abs(dm.dkdr2_truth(kid, x, 1.3) - fd) <= 1e-15 * abs(fd)
    z = np.linspace(-8.0, 8.0, 33)
    np.testing.assert_allclose([float(dm.norm_cdf(v)) for v in z], stats.norm.cdf(z), rtol=1e-14)
    np.testing.assert_allclose([float(dm.norm_pdf(v)) for v in z], stats.norm.pdf(z), rtol=1e-14)
    mu, s2, p0 = 0.7, 0.49, 0.2
    zz = (mu - p0) / 0.7
    assert abs(float(dm.acq_truth('ei', mu, s2, p0)) - ((mu - p0) * stats.norm.cdf(zz) + 0.7 * stats.norm.pdf(zz))) < 1e-15
    assert abs(float(dm.acq_truth('pi', mu, s2, p0)) - 0.5 * special.erfc(-zz / np.sqrt(2))) < 1e-15
    assert abs(float(dm.acq_truth('ucb', mu, s2, 4.0)) - (mu + 1.4)) <= 4.5e-16
    zc = np.linspace(-30, 30, 101)
    np.testing.assert_allclose([float(mp.cos(v)) for v in zc], np.cos(zc), rtol=0, atol=3e-16)
    # the dropped third term of cos_cw's pi, from the two doubles in the source
    assert 4.0e-21 < dm.C3 < 4.1e-21


def _nudge(v, ulps):
    return np.array([np.nextafter(x, np.inf) if ulps > 0 else x for x in v]) if ulps == 1 else \
        v + ulps * np.spacing(np.abs(v))


def test_covariance_checker_rejects_two_ulp():
    rng = np.random.RandomState(0)
    r2 = np.concatenate([10 ** rng.uniform(-8, 2.5, 60), rng.uniform(1400, 1480, 10)])
    for kid in range(4):
        exact = np.array([float(dm.kern_truth(kid, x, 1.0)) for x in r2])     # correctly rounded: passes
        bad, worst = dm.check_cov(kid, r2, exact)
        assert not bad.any() and worst <= 1.0, (kid, worst)
        sel = exact > 1e-300
        if kid == 0:
            off = exact + 2 * np.spacing(exact)                                # SE: 2 ulp is over its 1-ulp bound
            bad, _ = dm.check_cov(kid, r2[sel], off[sel])
            assert bad.all()
        else:
            # Matern: a relative error just over (3 + 2 s) eps
            s = np.array([float(dm._kern_s(kid, mp.mpf(x))[0]) for x in r2])
            off = exact * (1 + 1.01 * (3 + 2 * s) * dm.EPS) + 4 * np.spacing(exact)
            bad, _ = dm.check_cov(kid, r2[sel], off[sel])
            assert bad.all(), kid
    # past underflow: anything but 0 is rejected; an overflowed r2 (inf) must give 0, not NaN
    bad, _ = dm.check_cov(0, [1600.0, 1600.0], [0.0, 5e-324])
    assert list(bad) == [False, True]
    for kid in (1, 2):
        bad, _ = dm.check_cov(kid, [np.inf, 1.5e308, np.inf], [0.0, 0.0, np.nan])
        assert list(bad) == [False, False, True]
    bad, _ = dm.check_cov(0, [np.nan], [0.0])
    assert bad.all()


def test_cosine_checker_rejects_1e15():
    rng = np.random.RandomState(1)
    z = np.concatenate([rng.uniform(-32, 32, 100), (np.arange(1, 200) + 0.5) * np.pi])
    exact = np.array([float(mp.cos(v)) for v in z])
    assert not dm.check_cos(z, exact)[0].any()
    assert dm.check_cos(z, exact + 1e-15)[0].all()
    assert dm.check_cos(z, exact - 1e-15)[0].all()
    assert not dm.check_cos(z, exact, library=True)[0].any()
    assert dm.check_cos(z, exact + 1e-15, library=True)[0].all()


def test_gradient_and_acquisition_checkers_reject_small_errors():
    x = np.linspace(0.05, 5.0, 40)
    for kid in range(4):
        exact = np.array([float(2 * mp.mpf(v) * dm.dkdr2_truth(kid, v * v, 1.0)) for v in x])
        assert not dm.check_grad(kid, x, exact)[0].any()
        s = np.array([float(dm._kern_s(kid, mp.mpf(v * v))[0]) for v in x]) if kid else np.zeros_like(x)
        off = exact * (1 + 1.01 * ((3 + 2 * s) * dm.EPS + dm.U)) + 4 * np.sign(exact) * np.spacing(np.abs(exact))
        assert dm.check_grad(kid, x, off)[0].all(), kid
    mu = np.full(30, 0.5)
    s2 = np.full(30, 0.81)
    p0 = 0.5 - np.linspace(-30, 6, 30) * 0.9
    for acq in ('ei', 'pi'):
        exact = np.array([float(dm.acq_truth(acq, m, v, p)) for m, v, p in zip(mu, s2, p0)])
        assert not dm.check_acq(acq, mu, s2, p0, exact)[0].any()
        bound = np.array([dm.acq_bound(acq, m, v, p, dm.acq_truth(acq, m, v, p)) for m, v, p in zip(mu, s2, p0)])
        assert dm.check_acq(acq, mu, s2, p0, exact + 1.1 * bound + np.spacing(exact))[0].all()
    exact = np.array([float(dm.acq_truth('ucb', 0.3, 0.8, b)) for b in (0.0, 0.5, 2.0)])
    assert dm.check_acq('ucb', [0.3] * 3, [0.8] * 3, [0.0, 0.5, 2.0], exact + 4 * np.spacing(exact))[0].all()


def _exp_points():
    # x = -r2 / 2 spanning whole reduction intervals, densest next to r = -ln2/2 where the r^13 term is largest relative
    # to the result (|r|^13 / 13! = 1.8e-16 against p = 0.707)
    k = np.arange(-12, 0)
    edge = (k - 0.5) * np.log(2.0)
    x = np.concatenate([edge[:, None] + np.linspace(0, 2e-3, 25)[None, :], np.linspace(-20, 0, 200)[:, None]], axis=None)
    return np.sort(x)


def test_exp_nonpos_emulation_meets_the_se_bound_and_fails_it_without_its_r13_term():
    x = _exp_points()
    r2 = -2.0 * x
    full = np.array([dm.exp_nonpos_emul(v) for v in x])
    bad, worst = dm.check_cov(0, r2, full)
    assert not bad.any() and worst < 0.85, worst                 # the header's measured 0.79 ulp
    cut = np.array([dm.exp_nonpos_emul(v, [0.0] + dm.EXP_C[1:]) for v in x])
    bad, worst = dm.check_cov(0, r2, cut)
    assert bad.any() and worst > 1.2, worst
    # the subnormal tail and past underflow, through the emulation: <= one unit of 2^-1074, then exactly 0
    xs = np.linspace(-746.0, -708.0, 120)
    tail = np.array([dm.exp_nonpos_emul(v) for v in xs])
    assert not dm.check_cov(0, -2.0 * xs, tail)[0].any()


def test_cos_cw_emulation_meets_its_bound_and_fails_it_without_its_20th_power():
    k = np.arange(-60, 60)
    z = np.concatenate([(k + 0.5) * np.pi + np.linspace(-1e-6, 1e-6, 5)[:, None], np.linspace(-32, 32, 300)[:, None]],
                       axis=None)
    full = np.array([dm.cos_cw_emul(v) for v in z])
    bad, worst = dm.check_cos(z, full)
    assert not bad.any(), worst
    cut = np.array([dm.cos_cw_emul(v, [0.0] + dm.COS_C[1:]) for v in z])
    assert dm.check_cos(z, cut)[0].any()
    # far out the dropped third term of pi dominates: 2^20 pi has |n| C3 = 4.2e-15, over the old 3e-16 claim
    zb = np.array([(2.0 ** 20 + 0.5) * np.pi, 2.0 ** 20 * np.pi + 1.0])
    got = np.array([dm.cos_cw_emul(v) for v in zb])
    err = np.array([abs(float(mp.cos(mp.mpf(v)) - g)) for v, g in zip(zb, got)])
    assert err.max() > 3e-16
    assert not dm.check_cos(zb, got)[0].any()
