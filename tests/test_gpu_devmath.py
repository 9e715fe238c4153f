"""The hand-written device math (gpx_math.h exp_nonpos / sqrt_r2 / kern_eval, kernels_grad.hip kern_and_grad,
kernels_rff.hip cos_cw, kernels_sweep.hip k_acq) against 50-digit truth, through the library's own entry points.

Each probe is built so that every operation but the primitive under test is exact, so the library's output IS the
primitive's value at an argument the test chooses: d = 1, ell = 1, bias = 0, one observation at x = 0 and candidates
at x, so that the kernel's own r2 is fl(x * x).  With rho + sn2 = 4: L = 2, T = 1/2, y = 4 gives a = 2 and alpha = 1,
and mu = V.a = (k / 2) * 2 = k, k * alpha = k, dmu/dx = fl(g * 2x).  Truth and bounds: tests/devmath_ref.py (whose own
teeth are tested on the CPU in tests/test_devmath_cpu.py)."""
import numpy as np
import mpmath as mp
import pytest

import devmath_ref as dm

pytestmark = pytest.mark.gpu

KERNELS = ['se', 'matern5', 'matern3', 'matern1']
RHOS = [(1.0, 3.0), (1.3, 2.7)]


def _engine():
    from pybo_amd._lib import Engine
    return Engine(0)


def _probe(kernel, rho, sn2, ell=1.0):
    assert rho + sn2 == 4.0
    e = _engine()
    e.fit(np.zeros((1, 1)), np.array([4.0]), kernel, [ell], rho, sn2, 0.0)
    assert e.get_matrix('L')[0, 0] == 2.0 and e.get_matrix('T')[0, 0] == 0.5
    a, alpha = e.get_vectors()
    assert a[0] == 2.0 and alpha[0] == 1.0
    return e


def _r2(x, ell=1.0):
    xs = np.asarray(x, dtype=float) * (1.0 / ell)
    with np.errstate(over='ignore', invalid='ignore'):
        return xs * xs


def _x_for_r2(r2):
    """Coordinates whose fl(x * x) lands on (or next to) the wanted r2."""
    return np.sqrt(np.asarray(r2, dtype=float))


def _r2_sets(kernel):
    rng = np.random.RandomState(7)
    x_cut = 1e-140 * (1 + np.arange(-6, 7) * 2.0 ** -52)             # r2 = fl(x^2) next to the 1e-280 cutoff
    dense = 10 ** np.linspace(-16, 4, 1200)
    band = {'se': np.linspace(1400, 1500, 600), 'matern5': np.linspace(700, 750, 600) ** 2 / 5,
            'matern3': np.linspace(700, 750, 600) ** 2 / 3, 'matern1': np.linspace(700, 750, 600) ** 2}[kernel]
    x = np.concatenate([[0.0, 1e-160, 3e-158, 1e-155], x_cut, _x_for_r2(dense), _x_for_r2(band),
                        _x_for_r2(rng.uniform(0, 60, 100)), [1e150, 1e154, np.sqrt(1.5e308), 1e155, 1e200]])
    return x


def _kernel_band_check(kernel, r2, got, rho):
    bad, worst = dm.check_cov(dm.KIDS[kernel], r2, got, rho)
    assert not bad.any(), (kernel, rho, worst, list(zip(r2[bad][:6], got[bad][:6])))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# covariance: the Gram, every K* path, bitwise agreement, the bound, and the overflowed distance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
def test_covariance_paths_agree_bitwise_and_meet_the_bound(kernel):
    from pybo_amd._lib import Engine
    x = _r2_sets(kernel)
    r2 = _r2(x)
    for rho, sn2 in RHOS:
        # the Gram (k_gram_sym): stage 1 builds it without factorising, so a non-PD probe set is fine
        g = _engine()
        g.fit(np.concatenate([[0.0], x])[:, None], np.zeros(len(x) + 1), kernel, [1.0], rho, sn2, 0.0, stage=1)
        kg = g.get_matrix('K')[0, 1:]
        g.close()
        _kernel_band_check(kernel, r2, kg, rho)
        # the K* paths of the fitted probe
        e, e2 = _probe(kernel, rho, sn2), _probe(kernel, rho, sn2)
        X = x[:, None]
        half = 2.0 * (0.5 * kg)               # V = T k* = k / 2 rounds in the subnormal band: V.a = 2 fl(k / 2)
        paths = {
            'sweep': e.sweep('ei', 0.0, X, want_moments=True)['mu'],
            'predict': e.predict(X)[0],
            'predict_grad': e.predict(X, grad=True)[0],
            'predict_mean': e.predict_mean(X),
            'predict_mean_grad': e.predict_mean(X, grad=True)[0],
            'ensemble_predict': Engine.ensemble_predict([e, e2], X)[0],
            'ensemble_sweep_1': Engine.ensemble_sweep([e], 'mean', 0.0, X, want_moments=True)['mu'],
            'ensemble_sweep_2': Engine.ensemble_sweep([e, e2], 'mean', 0.0, X, want_moments=True)['mu'],
        }
        sel = np.arange(0, len(x), max(1, len(x) // 40))
        paths['predict_single'] = np.array([e.predict(X[i:i + 1], grad=True)[0][0] for i in sel])
        paths['predict_mean_single'] = np.array([e.predict_mean(X[i:i + 1], grad=True)[0][0] for i in sel])
        for name, got in paths.items():
            got = np.atleast_2d(got)
            want = kg[sel] if name.endswith('single') else kg
            alt = half[sel] if name.endswith('single') else half
            for row in got:
                ok = (row == want) | (row == alt)
                assert ok.all(), (kernel, rho, name, list(zip(r2[~ok][:5] if len(row) == len(r2) else [], row[~ok][:5],
                                                                  want[~ok][:5])))
        e.close()
        e2.close()


@pytest.mark.parametrize('kernel', KERNELS)
def test_overflowed_and_nan_distances(kernel):
    """r2 = +inf (and finite r2 >= 1.08e308, where (5/3) r2 used to overflow) gives 0, never NaN, for the value and for
    dk/dx; reached through a very small length scale as gpx_fit accepts it.  A NaN candidate gives NaN."""
    for ell in (1e-300, 1.0):
        e = _probe(kernel, 1.3, 2.7, ell=ell)
        if ell == 1.0:
            x = np.array([1e151, 1e154, np.sqrt(1.2e308), np.sqrt(1.7e308), 1e155, -1e200])
        else:
            x = np.array([1.0, 0.5, -2.0, 1.2e-146, 1.3e-146, 1e-149])
        r2 = _r2(x, ell)
        assert (r2 >= 1e300).all() and np.isinf(r2).any() and (np.isfinite(r2) & (r2 > 1.08e308)).any()
        X = x[:, None]
        for got in (e.sweep('ei', 0.0, X, want_moments=True)['mu'], e.predict(X)[0], e.predict_mean(X)):
            assert (got == 0.0).all(), (kernel, ell, got)
        g = _engine()
        g.fit(np.concatenate([[0.0], x])[:, None], np.zeros(len(x) + 1), kernel, [ell], 1.3, 2.7, 0.0, stage=1)
        assert (g.get_matrix('K')[0, 1:] == 0.0).all()
        g.close()
        if ell == 1.0:                          # (with ell = 1e-300 the chain-rule factor 2 / ell^2 is itself inf)
            for got in (e.predict_mean(X, grad=True)[1], e.predict(X, grad=True)[2]):
                assert (got == 0.0).all(), (kernel, got)
        mu = e.predict_mean(np.array([[np.nan]]))
        assert np.isnan(mu).all()
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
def test_gradient_paths_agree_bitwise_and_meet_the_bound(kernel):
    from pybo_amd._lib import Engine
    rng = np.random.RandomState(3)
    x = np.concatenate([10 ** np.linspace(-7, 2, 300), -10 ** np.linspace(-7, 1.5, 60), rng.uniform(-8, 8, 40)])
    if kernel == 'se':
        x = np.concatenate([x, np.sqrt(np.linspace(1400, 1490, 60))])
    else:
        c = {'matern5': np.sqrt(5), 'matern3': np.sqrt(3), 'matern1': 1.0}[kernel]
        x = np.concatenate([x, np.linspace(700, 744, 60) / c])
    X = x[:, None]
    for rho, sn2 in RHOS:
        e, e2 = _probe(kernel, rho, sn2), _probe(kernel, rho, sn2)
        base = e.predict_mean(X, grad=True)[1][:, 0]
        bad, worst = dm.check_grad(dm.KIDS[kernel], x, base, rho)
        assert not bad.any(), (kernel, rho, worst, list(zip(x[bad][:5], base[bad][:5])))
        others = {'predict': e.predict(X, grad=True)[2][:, 0],
                  'ensemble_predict': Engine.ensemble_predict([e, e2], X)[2][:, :, 0]}
        sel = np.arange(0, len(x), 9)
        others['predict_single'] = np.array([e.predict(X[i:i + 1], grad=True)[2][0, 0] for i in sel])
        others['predict_mean_single'] = np.array([e.predict_mean(X[i:i + 1], grad=True)[1][0, 0] for i in sel])
        for name, got in others.items():
            want = base[sel] if name.endswith('single') else base
            for row in np.atleast_2d(got):
                assert np.array_equal(row, want), (kernel, rho, name, np.flatnonzero(row != want)[:5])
        e.close()
        e2.close()


def test_matern12_gradient_is_zero_up_to_the_sqrt_cutoff_and_one_sided_beyond():
    """kern_and_grad's Matern-1/2 g = dk/dr2 is 0 at r = 0 (the symmetric value at the kink) and for every r2 <= 1e-280,
    where sqrt_r2 returns 0 (the candidate counts as sitting on the observation); above it dmu/dx is the one-sided
    -rho e^-r sign(x) (here within 1 ulp: e^-r = 1)."""
    e = _probe('matern1', 1.3, 2.7)
    x = 1e-140 * (1 + np.arange(-40, 41) * 2.0 ** -52)
    x = np.concatenate([x, -x, [0.0, -0.0, 1e-160, 1e-139, -1e-139, 1e-100]])
    r2 = _r2(x)
    dmu = e.predict_mean(x[:, None], grad=True)[1][:, 0]
    below = r2 <= 1e-280
    assert below.any() and (~below).any()
    assert (dmu[below] == 0.0).all()
    want = -1.3 * np.sign(x[~below])
    np.testing.assert_allclose(dmu[~below], want, rtol=2 * dm.EPS, atol=0)
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# cosines: cos_cw (Thompson sweep, n < 128 feature Gram) and the library cos (rff_eval_grad, n >= 128 feature Gram)
# ---------------------------------------------------------------------------------------------------------------------
def _cos_args():
    rng = np.random.RandomState(11)
    k = np.concatenate([np.arange(0, 200), np.unique(np.round(10 ** np.linspace(2.3, 4, 150)))])
    near = []
    for off in (-1e-9, 0.0, 3e-12):
        near.append((k + 0.5) * np.pi + off)
        near.append(k * np.pi + off)
    mags = 10 ** np.linspace(0, 9, 200) * np.where(np.arange(200) % 2, 1, -1)
    return np.concatenate([rng.uniform(-32, 32, 1500), np.concatenate(near), -np.concatenate(near)[::7], mags,
                           [0.0, -0.0, np.nan]])


def test_cosines_meet_their_bounds():
    z = _cos_args()
    e = _engine()
    e.fit(np.ones((1, 1)), np.array([1.0]), 'se', [1.0], 1.0, 0.1, 0.0)
    one = np.ones((1, 1, 1))
    # (a NaN candidate goes alone, as it did while the sweep's 4x4 MFMA tail let a NaN reach the candidates 4 rows away through a
    #  masking multiply; the tail adds a row's remainder terms without one now, tests/test_gpu_instantiations.py)
    fin = np.isfinite(z)
    v = np.full(len(z), np.nan)
    v[fin] = e.rff_sweep(one, np.zeros((1, 1)), np.ones((1, 1)), 0.0, z[fin, None])['vals'][0]
    v[~fin] = e.rff_sweep(one, np.zeros((1, 1)), np.ones((1, 1)), 0.0, z[~fin, None])['vals'][0]
    bad, worst = dm.check_cos(z, v)
    assert not bad.any(), ('cos_cw sweep', worst, list(zip(z[bad][:5], v[bad][:5])))
    f, g = e.rff_eval_grad(np.ones((1, 1)), np.zeros(1), np.ones(1), 0.0, z[:, None])
    bad, worst = dm.check_cos(z, f, library=True)
    assert not bad.any(), ('library cos', worst, list(zip(z[bad][:5], f[bad][:5])))
    bad, worst = dm.check_sin(z[fin], g[fin, 0])
    assert not bad.any(), ('library -sin', worst)
    # the feature Gram: one observation at x = 1, y - bias = 1, W = z, b = 0: v_j = cos(z_j)
    zf = z[np.isfinite(z)]
    zs = zf[np.linspace(0, len(zf) - 1, 400).astype(int)]
    S, n = 4, 100                                                      # n < 128: the MFMA feature path (cos_cw)
    _, vb = e.rff_gram_batch(zs.reshape(S, n, 1), np.zeros((S, n)))
    bad, worst = dm.check_cos(zs, vb.reshape(-1))
    assert not bad.any(), ('cos_cw feature Gram', worst)
    _, vw = e.rff_gram(zs[:300, None], np.zeros(300))                  # n >= 128: per-draw features (library cos)
    bad, worst = dm.check_cos(zs[:300], vw, library=True)
    assert not bad.any(), ('library cos feature Gram', worst)
    e.close()


@pytest.mark.parametrize('kernel', ['se', 'matern1'])
def test_thompson_value_of_both_cosines_agrees_on_a_realistic_draw(kernel):
    """rff_sweep (cos_cw, MFMA projection) against rff_eval_grad (library cos, FMA chain) on one posterior draw, d = 8.
    Per feature: the projections z differ by at most 2 gamma_{d+1} (|b| + sum |w x|) (two summation orders), which the
    cosine passes on 1:1; the cosines by cos_cw's bound + 2 ulp of the library's; the weighted sums over the n features by
    2 gamma_n sum |theta| (two orders).  That is ~1e-14 sum |theta| for SE, more where Matern-1/2's Cauchy-tailed W makes
    |z| large."""
    from oracle import gp_ref
    rng = np.random.RandomState(5)
    d, N, n = 8, 60, 100
    X = rng.rand(N, d)
    y = np.sin(X.sum(1))
    ell = 0.4 * np.ones(d)
    ref = gp_ref.make_gp(1e-3, 1.0, ell, 0.1, kernel)
    ref.add_data(X, y)
    smp = ref.sample_f(n, rng=9)
    e = _engine()
    e.fit(X, y, kernel, ell, 1.0, 1e-3, 0.1)
    Z = rng.rand(2000, d)
    vs = e.rff_sweep(smp.W[None], smp.b[None], smp.theta[None], 0.1, Z)['vals'][0]
    vg, _ = e.rff_eval_grad(smp.W, smp.b, smp.theta, 0.1, Z)
    proj = np.abs(Z) @ np.abs(smp.W).T + np.abs(smp.b)                 # (M, n)
    zz = Z @ smp.W.T + smp.b
    gam = lambda m: m * dm.U / (1 - m * dm.U)
    per = 2 * gam(d + 1) * proj + dm.COS_POLY_ABS + np.abs(dm.cos_cw_n(zz)) * dm.C3 + 4 * dm.U
    tol = per @ np.abs(smp.theta) + 2 * gam(n) * np.abs(smp.theta).sum() + 2 * dm.U * 0.1
    assert np.all(np.abs(vs - vg) <= tol), (np.max(np.abs(vs - vg) / tol), tol.max())
    assert tol.max() < 1e-13 * max(1.0, np.abs(smp.theta).sum()) * (1 if kernel == 'se' else 1e6)
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# acquisition lines of k_acq, at the device's own (mu, s2, p0)
# ---------------------------------------------------------------------------------------------------------------------
def test_acquisition_values_meet_their_bounds():
    e = _probe('se', 1.0, 3.0)
    X = np.linspace(0.0, 3.0, 48)[:, None]
    m = e.sweep('mean', 0.0, X, want_moments=True)
    mu, s2 = m['mu'], m['s2']
    s = np.sqrt(s2)
    for acq in ('ei', 'pi'):
        for z0 in np.linspace(-38, 8, 47):
            p0 = float(0.5 - z0 * 0.93)
            r = e.sweep(acq, p0, X, want_moments=True)
            assert np.array_equal(r['mu'], mu) and np.array_equal(r['s2'], s2)
            bad, worst = dm.check_acq(acq, mu, s2, p0, r['acq'])
            assert not bad.any(), (acq, z0, worst, ((mu - p0) / s)[bad][:4], r['acq'][bad][:4])
        # dlt = mu - p0 = 0 exactly: EI = s phi(0), PI = 1/2
        r = e.sweep(acq, float(mu[5]), X, want_moments=True)
        assert not dm.check_acq(acq, mu, s2, float(mu[5]), r['acq'])[0].any()
        if acq == 'pi':
            assert r['acq'][5] == 0.5
    for beta in (0.0, 0.5, 2.0, 1e3):
        r = e.sweep('ucb', beta, X, want_moments=True)
        bad, worst = dm.check_acq('ucb', mu, s2, beta, r['acq'])
        assert not bad.any(), ('ucb', beta, worst)
    e.close()
    # the s2 floor: rho = 1, sn2 = 1e-30 (K = 1 + 1e-30 = 1 in fp64): at the observation q = 1 and rho - q = 0 -> 1e-100
    f = _engine()
    f.fit(np.zeros((1, 1)), np.array([0.25]), 'se', [1.0], 1.0, 1e-30, 0.0)
    X0 = np.zeros((1, 1))
    m0 = f.sweep('mean', 0.0, X0, want_moments=True)
    assert m0['s2'][0] == 1e-100
    for acq in ('ei', 'pi'):
        for z0 in (-30.0, -5.0, 0.0, 3.0):
            p0 = float(m0['mu'][0] - z0 * 1e-50)
            r = f.sweep(acq, p0, X0, want_moments=True)
            assert not dm.check_acq(acq, m0['mu'], m0['s2'], p0, r['acq'])[0].any(), (acq, z0, r['acq'])
    f.close()
