"""Pathwise Thompson draws on the device (gpx_path_weights / gpx_path_sweep[_dev] / gpx_path_grad; kernels_path.hip) against the numpy
restatement tests/path_ref.py.  The tolerances are path_ref's: the residual bar tests/test_gpu_configs.py holds alpha to, and for values
and gradients (nv + n + 64) 2^-53 times the sum of the absolute terms plus the feature part's own bar.  The shapes are the smallest at
which the kernels can go wrong: N = 300 (five 64-row tiles, the last partial), 129 (a second 128-block of one row, d = 20: the staged
coordinate chunks) and 1; S = 1, 5, 65 (one block, a partial block, a second group of one draw); n = 100 and 130 (a second feature tile);
M = 1000 (eight workgroups, the last partial)."""

import numpy as np
import pytest

import path_ref
from oracle import gp_ref

pytestmark = pytest.mark.gpu

CASES = {'n300_d3': (300, 3, 100, 5, 1e-4), 'n129_d20': (129, 20, 130, 3, 1e-6), 'n1_d2': (1, 2, 100, 2, 1e-2)}
M = 1000
_CACHE = {}


def _model(case, kernel):
    N, d, n, S, snr = CASES[case]
    return path_ref.model(N, d, 11 + N, snr, kernel)


def _engine(m, rows=None):
    from pybo_amd import _lib
    e = _lib.Engine(0)
    X, y = (m['X'], m['y']) if rows is None else (m['X'][:rows], m['y'][:rows])
    e.fit(X, y, m['kernel'], m['ell'], m['rho'], m['sn2'], m['bias'])
    return e


def _draws(m, n, S, seed, nv=None):
    """Spectral draws and, from the reference, the weights of S draws conditioned on the leading nv observations (computed once)."""
    key = (m['kernel'], len(m['X']), n, S, seed, nv)
    if key not in _CACHE:
        X, y = (m['X'], m['y']) if nv is None else (m['X'][:nv], m['y'][:nv])
        W, b, w = path_ref.spectral(m['kernel'], n, X.shape[1], m['ell'], S, seed)
        eps = np.random.RandomState(seed + 1).randn(S, len(X))
        sc = np.sqrt(2.0 * m['rho'] / n)
        theta, v, r, Kn = path_ref.weights(m['kernel'], X, y, m['ell'], m['rho'], m['sn2'], m['bias'], W, b, w, eps, sc)
        _CACHE[key] = dict(W=W, b=b, w=w, eps=eps, sc=sc, theta=theta, v=v, r=r, Kn=Kn)
    return _CACHE[key]


def _cands(d, seed=3):
    return np.random.RandomState(seed).rand(M, d)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# 1. weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', path_ref.KERNELS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_weights_solve_the_system_to_the_bar_alpha_is_held_to(case, kernel):
    N, d, n, S, _ = CASES[case]
    m = _model(case, kernel)
    D = _draws(m, n, S, 5)
    e = _engine(m)
    try:
        theta, v = e.path_weights(D['W'], D['b'], D['w'], D['eps'], D['sc'])
        assert _bits(theta, D['sc'] * D['w'])
        res = np.linalg.norm(v @ D['Kn'] - D['r'], axis=1)
        tol = path_ref.resid_tol(D['Kn'], v, D['r'])
        print(case, kernel, 'residual / bar', res / tol)
        assert np.all(res <= tol)
        # w = 0, no noise draw: the right-hand side is y - bias itself, the solution alpha
        theta0, v0 = e.path_weights(D['W'], D['b'], np.zeros_like(D['w']), None, D['sc'])
        assert not theta0.any()
        alpha = e.get_vectors()[1]
        r0 = np.tile(m['y'] - m['bias'], (S, 1))
        tol0 = path_ref.resid_tol(D['Kn'], v0, r0)
        assert np.all(np.linalg.norm(v0 @ D['Kn'] - r0, axis=1) <= tol0)
        tola = path_ref.resid_tol(D['Kn'], alpha, r0[0])
        assert np.all(np.linalg.norm((v0 - alpha) @ D['Kn'], axis=1) <= tol0 + tola)      # (each is within its bar of the same right-hand side)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sweep's values, its top-k, host against device variant
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', path_ref.KERNELS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_sweep_values_topk_and_the_device_variant(case, kernel):
    from test_gpu_prune import _DevBuf, _dev
    N, d = CASES[case][:2]
    m = _model(case, kernel)
    Xc = _cands(d)
    dXc = _dev(Xc)
    e = _engine(m)
    try:
        for S in (1, 5, 65):
            for n in (100, 130):
                for nv in ((N, 200) if N == 300 else (N,)):
                    D = _draws(m, n, S, 7, None if nv == N else nv)
                    out = e.path_sweep(D['W'], D['b'], D['theta'], D['v'], m['bias'], Xc, k=10)
                    f, B = path_ref.values(kernel, m['X'][:nv], m['ell'], m['rho'], m['bias'], D['W'], D['b'], D['theta'], D['v'], Xc)
                    tol = path_ref.value_tol(B, f, nv, n, m['rho'])
                    err = np.abs(out['vals'] - f)
                    print(case, kernel, 'S', S, 'n', n, 'nv', nv, 'max err / tol', (err / tol).max())
                    assert np.all(err <= tol)
                    for s in range(S):
                        order = gp_ref.topk_desc(out['vals'][s], 10)
                        assert np.array_equal(out['top_idx'][s], order) and _bits(out['top_val'][s], out['vals'][s][order])
                    buf = _DevBuf(S * M)
                    tv, ti = e.path_sweep_dev(D['W'], D['b'], D['theta'], D['v'], m['bias'], dXc.data_ptr(), M, 10, d_vals=buf.data_ptr())
                    e.sync()
                    assert _bits(buf.numpy().reshape(S, M), out['vals']) and _bits(tv, out['top_val']) and np.array_equal(ti, out['top_idx'])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a draw's value depends on its weights and the candidate alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['se', 'matern1'])
@pytest.mark.parametrize('case', ['n300_d3', 'n129_d20'])
def test_a_value_does_not_depend_on_the_other_draws_or_candidates(case, kernel):
    N, d = CASES[case][:2]
    m = _model(case, kernel)
    D = _draws(m, 100, 65, 7)
    Xc = _cands(d)
    e = _engine(m)
    try:
        def sweep(sel, X):
            return e.path_sweep(D['W'][sel], D['b'][sel], D['theta'][sel], D['v'][sel], m['bias'], X, k=0)['vals']
        full = sweep(slice(0, 65), Xc)
        assert _bits(sweep(slice(0, 1), Xc)[0], full[0])           # draw 0 of 65 = the draw alone
        assert _bits(sweep(slice(64, 65), Xc)[0], full[64])        # the second group's only draw = the draw alone
        assert _bits(sweep(slice(0, 65), Xc[:130]), full[:, :130])  # the first 130 candidates alone
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the conditioning identity: K (K + sn2 I)^-1 = I - sn2 (K + sn2 I)^-1, so f_s(X_i) = y_i - sqrt(sn2) eps_si - sn2 v_si
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', path_ref.KERNELS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_a_draw_passes_through_the_data_up_to_its_noise(case, kernel):
    N, d, n, S, _ = CASES[case]
    m = _model(case, kernel)
    D = _draws(m, n, S, 5)
    e = _engine(m)
    try:
        theta, v = e.path_weights(D['W'], D['b'], D['w'], D['eps'], D['sc'])
        got = e.path_sweep(D['W'], D['b'], theta, v, m['bias'], m['X'], k=0)['vals']
        want = m['y'][None, :] - np.sqrt(m['sn2']) * D['eps'] - m['sn2'] * v
        f, B = path_ref.values(kernel, m['X'], m['ell'], m['rho'], m['bias'], D['W'], D['b'], theta, v, m['X'])
        tol = path_ref.value_tol(B, f, N, n, m['rho']) + path_ref.resid_tol(D['Kn'], v, D['r'])[:, None]
        err = np.abs(got - want)
        print(case, kernel, 'max err / tol', (err / tol).max())
        assert np.all(err <= tol)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. no prior, no noise: the posterior mean
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', path_ref.KERNELS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_without_prior_and_noise_the_draw_is_the_posterior_mean(case, kernel):
    from helpers import mu_tol
    N, d, n, S, _ = CASES[case]
    m = _model(case, kernel)
    D = _draws(m, n, S, 5)
    Xc = _cands(d)[:300]
    e = _engine(m)
    try:
        theta0, v0 = e.path_weights(D['W'], D['b'], np.zeros_like(D['w']), None, D['sc'])
        got = e.path_sweep(D['W'], D['b'], theta0, v0, m['bias'], Xc, k=0)['vals']
        mu = e.predict_mean(Xc)
        assert np.all(np.abs(got - mu[None, :]) <= mu_tol(mu, m['rho'])[None, :])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. value and gradient of one draw
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', path_ref.KERNELS)
@pytest.mark.parametrize('case', ['n300_d3', 'n129_d20'])
def test_value_and_gradient_of_one_draw(case, kernel):
    N, d, n, S, _ = CASES[case]
    m = _model(case, kernel)
    D = _draws(m, n, S, 5)
    W, b, theta, v = D['W'][1], D['b'][1], D['theta'][1], D['v'][1]
    e = _engine(m)
    try:
        for npts in (1, 7, 130):
            Xc = _cands(d, seed=9)[:npts].copy()
            if npts > 1:
                Xc[1] = m['X'][N // 2]                       # on top of an observation: Matern-1/2's kink, whose gradient is defined as 0
            f, g = e.path_eval_grad(W, b, theta, v, m['bias'], Xc)
            rf, rg, Bf, Bg = path_ref.value_grad(kernel, m['X'], m['ell'], m['rho'], m['bias'], W, b, theta, v, Xc)
            tf, tg = path_ref.value_tol(Bf, rf, N, n, m['rho']), path_ref.grad_tol(Bg, rg, N, n, m['rho'], m['ell'])
            print(case, kernel, npts, 'f err / tol', (np.abs(f - rf) / tf).max(), 'g err / tol', (np.abs(g - rg) / tg).max())
            assert np.all(np.abs(f - rf) <= tf) and np.all(np.abs(g - rg) <= tg)
            # ... and the sweep's value of the same draw
            sw = e.path_sweep(W[None], b[None], theta[None], v[None], m['bias'], Xc, k=0)['vals'][0]
            assert np.all(np.abs(f - sw) <= 2.0 * tf)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. a handle with a history
# ---------------------------------------------------------------------------------------------------------------------
def test_a_draw_survives_appends_and_leaves_the_sweep_cache_alone():
    from test_gpu_prune import _dev
    m = path_ref.model(129, 3, 21, 1e-4, 'matern5')
    D = _draws(dict(m, X=m['X'][:127], y=m['y'][:127]), 100, 5, 5)
    Xc = _cands(3)
    dXc = _dev(Xc)

    def history(with_path):
        """fit 127, cache a sweep, [weights + path sweep], append twice, [path sweep with the old v], re-score the cache"""
        e = _engine(m, rows=127)
        try:
            e.set_option('sweep_cache', 1)
            cold = e.sweep_dev('ei', 0.3, dXc.data_ptr(), M, 10)
            e.set_option('sweep_cache', 0)
            seen = []
            if with_path:
                theta, v = e.path_weights(D['W'], D['b'], D['w'], D['eps'], D['sc'])
                seen.append(e.path_sweep(D['W'], D['b'], theta, v, m['bias'], Xc, k=10))
            for i in (127, 128):
                assert e.append(m['X'][i], m['y'][i])
            if with_path:
                seen.append(e.path_sweep(D['W'], D['b'], theta, v, m['bias'], Xc, k=10))
                assert e.path_eval_grad(D['W'][0], D['b'][0], theta[0], v[0], m['bias'], Xc[:3])[0].shape == (3,)
            assert e.sweep_cache_size() == M
            warm = e.sweep_update('ei', 0.3, k=10, want_moments=True)
            return cold, seen, warm
        finally:
            e.close()
    cold, seen, warm = history(True)
    for key in ('vals', 'top_val'):
        assert _bits(seen[0][key], seen[1][key])                    # N = 129, a new 128-block: the same function of the leading 127 rows
    assert np.array_equal(seen[0]['top_idx'], seen[1]['top_idx'])
    cold0, _, warm0 = history(False)
    assert _bits(cold[0], cold0[0]) and np.array_equal(cold[1], cold0[1])
    for key in ('acq', 'mu', 's2', 'top_val'):
        assert _bits(warm[key], warm0[key]), key
    assert np.array_equal(warm['top_idx'], warm0['top_idx'])


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors leave the handle usable
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_reported_and_leave_the_handle_usable():
    from pybo_amd import _lib
    m = _model('n300_d3', 'se')
    D = _draws(m, 100, 5, 7)
    N, d, S, n = 300, 3, 5, 100
    Xc = _cands(d)
    lib = _lib.load()
    p = _lib._ptr
    f64 = np.ascontiguousarray
    W, b, th, v, w = f64(D['W']), f64(D['b']), f64(D['theta']), f64(D['v']), f64(D['w'])
    tv, ti, out = np.empty((S, 10)), np.empty((S, 10), dtype=np.int64), np.empty((S, M))
    fo, go = np.empty(4097), np.empty((4097, d))
    big = f64(np.zeros((4097, d)))

    def sweep(h, W=W, nv=N, S=S, n=n, d=d, k=10):
        return lib.gpx_path_sweep(h, p(W), p(b), p(th), p(v), nv, S, n, d, m['bias'], p(Xc), M, k, p(tv), p(ti), p(out))

    def grad(h, nv=N, n=n, d=d, Mg=3):
        return lib.gpx_path_grad(h, p(W), p(b), p(th), p(v), nv, n, d, m['bias'], p(big), Mg, p(fo), p(go))

    def wts(h, S=S, n=n):
        return lib.gpx_path_weights(h, p(W), p(b), p(w), None, S, n, D['sc'], p(np.empty((5, 100))), p(np.empty((5, N))))

    fresh = _lib.Engine(0)
    try:
        assert sweep(fresh._h) == _lib.GPX_ESTATE and grad(fresh._h) == _lib.GPX_ESTATE and wts(fresh._h) == _lib.GPX_ESTATE
        fresh.fit(m['X'], m['y'], 'se', m['ell'], m['rho'], m['sn2'], m['bias'])       # ... and the handle still fits and sweeps
        assert sweep(fresh._h) == 0
    finally:
        fresh.close()
    e = _engine(m)
    try:
        good = e.path_sweep(W, b, th, v, m['bias'], Xc, k=10)
        h = e._h
        for rc in (sweep(h, d=2), sweep(h, nv=0), sweep(h, nv=N + 1), sweep(h, S=0), sweep(h, n=0), sweep(h, n=4097), sweep(h, k=4097),
                   grad(h, d=2), grad(h, nv=0), grad(h, nv=N + 1), grad(h, n=0), grad(h, n=4097), grad(h, Mg=4097), grad(h, Mg=0),
                   wts(h, S=0), wts(h, n=0), wts(h, n=4097)):
            assert rc == _lib.GPX_EARG
            assert lib.gpx_last_error(h)
        dev = lib.gpx_path_sweep_dev(h, p(W), p(b), p(th), p(v), N, S, n, d, m['bias'], None, M, 4097, p(tv), p(ti), None)
        assert dev == _lib.GPX_EARG
        again = e.path_sweep(W, b, th, v, m['bias'], Xc, k=10)
        assert _bits(again['vals'], good['vals']) and np.array_equal(again['top_idx'], good['top_idx'])
        assert grad(h) == 0 and wts(h) == 0
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_the_model_the_policy_and_the_loop():
    from pybo_amd import models, policies, solve_bayesopt
    from pybo_amd._lib import DeviceGrid
    from pybo_amd.models.gp import PathSampleDevice, RFFSampleDevice
    m = path_ref.model(60, 2, 4, 1e-3, 'matern5')
    gp = models.make_gp(m['sn2'], m['rho'], m['ell'], m['bias'], kernel='matern5')
    assert isinstance(gp.sample_f(100, rng=0, method='pathwise'), RFFSampleDevice)       # no data: the prior sample, as 'rff'
    gp.add_data(m['X'], m['y'])
    rff, path = gp.sample_f(100, rng=0), gp.sample_f(100, rng=0, method='pathwise')
    assert isinstance(path, PathSampleDevice) and isinstance(rff, RFFSampleDevice) and not isinstance(rff, PathSampleDevice)
    assert _bits(path.W, rff.W) and _bits(path.b, rff.b) and path.nv == 60 and path.bias == m['bias']
    with pytest.raises(ValueError):
        gp.sample_f(100, rng=0, method='exact')
    # .get against .topk on a host grid and a DeviceGrid
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    grid = DeviceGrid('uniform', bounds, 1500, seed=2)
    Z = np.asarray(grid)
    vals = path.get(Z)
    order = gp_ref.topk_desc(vals, 5)
    for g in (Z, grid):
        tv, ti = path.topk(g, 5)
        assert np.array_equal(ti, order) and _bits(tv, vals[order])
    assert _bits(path(Z[:9]), vals[:9])
    # .get(x, grad=True) agrees with .get
    f, g = path.get(Z[:7], grad=True)
    rf, rg, Bf, Bg = path_ref.value_grad('matern5', m['X'], m['ell'], m['rho'], m['bias'], path.W, path.b, path.theta, path.v, Z[:7])
    assert np.all(np.abs(f - vals[:7]) <= 2.0 * path_ref.value_tol(Bf, rf, 60, 100, m['rho']))
    assert np.all(np.abs(g - rg) <= path_ref.grad_tol(Bg, rg, 60, 100, m['rho'], m['ell']))
    # it survives an append unchanged in bits ...
    gp.add_data(np.array([[0.31, 0.77]]), np.array([0.4]))
    assert gp.ndata == 61 and _bits(path.get(Z), vals)
    # ... a fresh sample sees the new point, and a hyper-parameter change is refused
    assert gp.sample_f(100, rng=0, method='pathwise').nv == 61
    gp.rho = 2.0 * gp.rho
    with pytest.raises(RuntimeError):
        path.get(Z[:3])
    with pytest.raises(RuntimeError):
        path.topk(grid, 3)
    gp.rho = m['rho']
    assert _bits(path.get(Z[:9]), vals[:9])
    other = models.make_gp(m['sn2'], m['rho'], m['ell'], m['bias'], kernel='matern5')
    other.add_data(m['X'][::-1], m['y'][::-1])
    stale = PathSampleDevice(other, path.W, path.b, path.theta, path.v[:60])
    stale._X = m['X']
    with pytest.raises(RuntimeError):
        stale.get(Z[:3])
    grid.close()
    # the policy, the ensemble, the sharded model, the loop
    index = policies.Thompson(gp, None, None, n=50, rng=1, method='pathwise')
    assert hasattr(index, 'topk') and index(Z[:4]).shape == (4,)
    ens = models.MCMC(gp, n=2, burn=2, rng=0)
    assert isinstance(ens.sample_f(50, rng=0, method='pathwise'), PathSampleDevice)
    assert not isinstance(ens.sample_f(50, rng=0), PathSampleDevice)
    sharded = models.make_gp(m['sn2'], m['rho'], m['ell'], m['bias'], kernel='matern5', devices=[0])
    sharded.add_data(m['X'], m['y'])
    with pytest.raises(NotImplementedError):
        sharded.sample_f(50, rng=0, method='pathwise')
    box = np.array([[-1.0, 1.0], [-1.0, 1.0]])
    start = models.make_gp(1e-4, 1.0, [0.5, 0.5], 0.0)
    xbest, model, info = solve_bayesopt(lambda x: -float(np.sum((np.ravel(x) - 0.3) ** 2)), box, model=start, niter=5,
                                        policy=('thompson', {'method': 'pathwise'}), solver=('lbfgs', {'ngrid': 500, 'nbest': 3}), rng=0)
    assert np.all(xbest >= box[:, 0]) and np.all(xbest <= box[:, 1]) and len(info.y) >= 5
