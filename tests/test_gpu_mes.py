"""Max-value entropy search on the device (GPX_ACQ_MES = 16: pybo_amd/csrc/mes_math.h, kernels_mes.hip) against the 50-digit truth and the
derived bound of tests/mes_ref.py, through every entry that accepts it, and what refuses it.

Shapes: N = 200 (two 128-blocks, the second partial), d = 3, M = 1000 (a multiple of neither 128 nor 256), S in {1, 7, 64}, SE and
Matern-5/2.  The moments a MES sweep returns are array-equal to a 'mean' sweep's throughout: k_acq_mes forms them by k_acq's statements."""
import numpy as np
import pytest

import mes_ref
from oracle import gp_ref
from helpers import synth_problem, s2_tol, mu_tol
from pybo_amd.mes import mes_value

pytestmark = pytest.mark.gpu

N, D, M = 200, 3, 1000
RHO, SN2, BIAS = 1.3, 1e-3, 0.2
KERNELS = ['se', 'matern5']
_CACHE = {}


def _engine():
    from pybo_amd._lib import Engine
    return Engine(0)


def _problem():
    if 'p' not in _CACHE:
        X, y, ell = synth_problem(N + 2, D, seed=21)
        ell = 0.35 * ell            # short length scales: the posterior variance spans 2e-3 .. 1.2, the values stay within a decade
        Z = np.random.RandomState(8).rand(M, D)
        rng = np.random.RandomState(13)
        ys = {S: y[:N].max() + 0.05 + 0.8 * rng.rand(S) for S in (1, 7, 64)}
        _CACHE['p'] = dict(X=X, y=y, ell=ell, Z=Z, ys=ys)
    return _CACHE['p']


def _fitted(kernel, n=N, ell=None):
    p = _problem()
    e = _engine()
    e.fit(p['X'][:n], p['y'][:n], kernel, p['ell'] if ell is None else ell, RHO, SN2, BIAS)
    return e


def _mean(kernel):
    """The 'mean' sweep's moments over Z (once per kernel): what every MES sweep must return bit for bit."""
    if ('m', kernel) not in _CACHE:
        e = _fitted(kernel)
        r = e.sweep('mean', None, _problem()['Z'], want_moments=True)
        e.close()
        _CACHE[('m', kernel)] = (r['mu'], r['s2'])
    return _CACHE[('m', kernel)]


def _within(mu, s2, ys, got, rows):
    bad, worst = mes_ref.check_mes(mu[rows], s2[rows], ys[rows] if np.ndim(ys) == 2 else ys, got[rows])
    assert not bad.any(), (worst, rows[bad][:5], got[rows][bad][:5])
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# device math at the device's own moments (the probe of tests/test_gpu_devmath.py)
# ---------------------------------------------------------------------------------------------------------------------
GAMMAS = np.concatenate([-np.logspace(0, 6, 19), -np.linspace(7.9, 8.1, 5), -np.linspace(0.0, 7.0, 8), [-0.0, 1e-12],
                         np.linspace(0.5, 7.5, 8), np.linspace(7.9, 8.1, 5), np.linspace(9.0, 37.0, 12), [37.6, 38.0, 38.5, 38.9, 39.5]])


def test_device_math_meets_the_bound_at_the_devices_own_moments():
    assert len(GAMMAS) == 64 and GAMMAS.min() == -1e6
    e = _engine()
    e.fit(np.zeros((1, 1)), np.array([4.0]), 'se', [1.0], 1.0, 3.0, 0.0)
    X = np.linspace(0.0, 3.0, 48)[:, None]
    m = e.sweep('mean', 0.0, X, want_moments=True)
    mu, s2 = m['mu'], m['s2']
    s = np.sqrt(s2)
    rows = np.array([0, 5, 11, 23, 40, 47])
    worst = 0.0
    for g0 in GAMMAS:
        j = 5
        ystar = np.array([float(mu[j] + g0 * s[j])])
        r = e.sweep('mes', ystar, X, want_moments=True)
        assert np.array_equal(r['mu'], mu) and np.array_equal(r['s2'], s2)
        v = r['acq']
        assert np.all(v >= 0.0) and not np.signbit(v).any() and np.isfinite(v).all(), (g0, v)
        worst = max(worst, _within(mu, s2, ystar, v, rows))
    print('worst error / bound over the probe: %.3f' % worst)
    # a NaN candidate: NaN moment -> NaN value, ranked last
    Xn = X.copy()
    Xn[7, 0] = np.nan
    r = e.sweep('mes', np.array([float(mu[5] + s[5])]), Xn, k=48, want_moments=True)
    assert np.isnan(r['mu'][7]) and np.isnan(r['acq'][7]) and np.isfinite(np.delete(r['acq'], 7)).all()
    assert r['top_idx'][-1] == 7 and not r['top_val'][-1] > -np.inf         # (as for every acquisition: last, reported as -inf)
    assert sorted(r['top_idx'][:-1].tolist()) == [i for i in range(48) if i != 7] and np.all(np.diff(r['top_val'][:-1]) <= 0.0)
    e.close()
    # the s2 floor: rho = 1, sn2 = 1e-30 (K = 1 + 1e-30 = 1 in fp64): at the observation q = 1 and rho - q = 0 -> 1e-100
    f = _engine()
    f.fit(np.zeros((1, 1)), np.array([0.25]), 'se', [1.0], 1.0, 1e-30, 0.0)
    X0 = np.zeros((1, 1))
    m0 = f.sweep('mean', 0.0, X0, want_moments=True)
    assert m0['s2'][0] == 1e-100
    for g0 in (-1e6, -30.0, -5.0, 0.0, 3.0, 30.0):
        ystar = np.array([float(m0['mu'][0] + g0 * 1e-50)])
        r = f.sweep('mes', ystar, X0, want_moments=True)
        assert r['s2'][0] == 1e-100 and r['mu'][0] == m0['mu'][0]
        _within(m0['mu'], m0['s2'], ystar, r['acq'], np.array([0]))
    # gamma = -+inf from FINITE maxima (an infinite y* is refused): (y* - mu) / 1e-50 overflows
    lo = f.sweep('mes', np.array([-1e300]), X0)['acq'][0]
    hi = f.sweep('mes', np.array([1e300]), X0)['acq'][0]
    assert lo == np.inf and hi == 0.0 and not np.signbit(hi)
    both = f.sweep('mes', np.array([1e300, -1e300, 1e300]), X0)['acq'][0]
    assert both == np.inf                                   # (an infinite term: the sum itself, not the carried roundings' NaN)
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# the summation rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
def test_summation_rule(kernel):
    p = _problem()
    mu, s2 = _mean(kernel)
    e = _fitted(kernel)
    y = float(p['ys'][1][0])
    one = e.sweep('mes', np.array([y]), p['Z'], want_moments=True)
    assert np.array_equal(one['mu'], mu) and np.array_equal(one['s2'], s2)
    for S in (2, 4, 64):
        assert np.array_equal(e.sweep('mes', np.full(S, y), p['Z'])['acq'], one['acq']), S
    rows = np.arange(0, M, 9)
    _within(mu, s2, np.array([y]), one['acq'], rows)
    seven = e.sweep('mes', p['ys'][7], p['Z'])['acq']
    _within(mu, s2, p['ys'][7], seven, rows)
    # ... and the numpy closure on the same moments is the same number to within the bound's two sides
    ref = mes_value(mu, s2, p['ys'][7])
    tol = np.array([2 * mes_ref.mes_bound(mu[i], s2[i], p['ys'][7]) for i in rows])
    assert np.all(np.abs(seven[rows] - ref[rows]) <= tol)
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('S', [1, 7, 64])
def test_every_path_returns_the_same_values_and_the_topk_is_theirs(kernel, S):
    from test_gpu_prune import _DevBuf, _dev
    p = _problem()
    mu, s2 = _mean(kernel)
    ys = p['ys'][S]
    e = _fitted(kernel)
    host = e.sweep('mes', ys, p['Z'], k=64, want_moments=True)
    assert np.array_equal(host['mu'], mu) and np.array_equal(host['s2'], s2)
    vals = host['acq']
    dZ, buf = _dev(p['Z']), _DevBuf(M)
    tv, ti = e.sweep_dev('mes', ys, dZ.data_ptr(), M, 64, d_acq=buf.data_ptr())
    e.sync()
    assert np.array_equal(buf.numpy(), vals) and np.array_equal(tv, host['top_val']) and np.array_equal(ti, host['top_idx'])
    e.set_option('chunk', 128)
    assert np.array_equal(e.sweep('mes', ys, p['Z'])['acq'], vals)
    # the reference: the numpy closure on the moments the device returned.  Precondition for comparing ORDERS: its k + 1 best are
    # separated by more than 1000 bounds (seeds 21 / 8 / 13 were chosen on the CPU so that they are: by 6e9 bounds on the oracle's moments)
    ref = mes_value(mu, s2, ys)
    order = gp_ref.topk_desc(ref, 65)
    rel = max(mes_ref.mes_bound(mu[i], s2[i], ys) / ref[i] for i in order[::8])         # (relative: every ninth of the 65)
    gaps = -np.diff(ref[order])
    assert np.all(gaps > 1000 * rel * ref[order[:-1]]), (np.min(gaps / ref[order[:-1]]), rel)
    for k in (1, 10, 64):
        r = e.sweep('mes', ys, p['Z'], k=k, want_all=False)
        want = gp_ref.topk_desc(vals, k)
        assert np.array_equal(r['top_idx'], want) and np.array_equal(r['top_val'], vals[want])
        assert np.array_equal(r['top_idx'], order[:k])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# warm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
def test_warm_rescore(kernel):
    p = _problem()
    ys = p['ys'][7]
    e = _fitted(kernel)
    e.set_option('sweep_cache', 1)
    cold0 = e.sweep('mes', ys, p['Z'], k=5, want_moments=True)
    e.set_option('sweep_cache', 0)
    assert e.sweep_cache_size() == M
    same = e.sweep_update('mes', ys, k=5, want_moments=True)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        assert np.array_equal(same[key], cold0[key]), key          # re-scoring the untouched sums: bitwise
    for i in (N, N + 1):
        assert e.append(p['X'][i], p['y'][i])
    warm = e.sweep_update('mes', ys, k=5, want_moments=True)
    rows = np.arange(0, M, 9)
    _within(warm['mu'], warm['s2'], ys, warm['acq'], rows)      # the value at the moments IT returns
    want = gp_ref.topk_desc(warm['acq'], 5)
    assert np.array_equal(warm['top_idx'], want)
    ce = _fitted(kernel, n=N + 2)
    cold = ce.sweep('mean', None, p['Z'], want_moments=True)
    ce.close()
    assert np.all(np.abs(warm['s2'] - cold['s2']) <= 0.01 * s2_tol(cold['s2'], RHO))
    assert np.all(np.abs(warm['mu'] - cold['mu']) <= 0.01 * mu_tol(cold['mu'], RHO))
    # other maxima: O(M), no sweep launch (timer slot 8), the same moments
    t0 = e.timers()
    other = e.sweep_update('mes', ys[:3] + 0.25, k=5, want_moments=True)
    t1 = e.timers()
    assert t1['sweep_trmm_launches'] == t0['sweep_trmm_launches'] and t1['rank1'] == t0['rank1']
    assert np.array_equal(other['mu'], warm['mu']) and np.array_equal(other['s2'], warm['s2'])
    _within(other['mu'], other['s2'], ys[:3] + 0.25, other['acq'], rows)
    assert not np.array_equal(other['acq'], warm['acq'])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# ensemble
# ---------------------------------------------------------------------------------------------------------------------
def test_ensemble_layout_and_refusals():
    """The value is ((v_0 + v_1) + v_2) / 3 of the members' single sweeps, each with ITS slice of the member-major maxima: array-equal
    (the ensemble's add and divide run with contraction off, kernels_ens.hip)."""
    from pybo_amd._lib import Engine, GpxError, GPX_EARG
    p = _problem()
    ells = [p['ell'], 0.7 * p['ell'], 1.4 * p['ell']]
    engines = [_fitted('se', ell=l) for l in ells]
    for S in (1, 7):
        ys = np.array([p['ys'][7][:S] + 0.1 * m for m in range(3)])
        got = Engine.ensemble_sweep(engines, 'mes', ys, p['Z'], k=10)
        singles = [e.sweep('mes', ys[m], p['Z'])['acq'] for m, e in enumerate(engines)]
        want = ((singles[0] + singles[1]) + singles[2]) / 3.0
        assert np.array_equal(got['acq'], want)
        assert np.array_equal(got['top_idx'], gp_ref.topk_desc(want, 10))
        swapped = Engine.ensemble_sweep(engines, 'mes', ys[::-1], p['Z'])['acq']
        assert not np.array_equal(swapped, want)                # the slices belong to their members
    one = Engine.ensemble_sweep(engines[:1], 'mes', p['ys'][64], p['Z'])['acq']
    assert np.array_equal(one, engines[0].sweep('mes', p['ys'][64], p['Z'])['acq'])
    for bad in (np.ones(7), np.ones(2), np.ones(3 * 65), np.zeros(0)):
        with pytest.raises(GpxError, match=r'ensemble_sweep: MES takes n_members \* S maximum samples, S in \[1, 64\]') as err:
            Engine.ensemble_sweep(engines, 'mes', bad, p['Z'])
        assert err.value.code == GPX_EARG
    with pytest.raises(GpxError, match='ensemble_sweep: MES takes 1 to 64 finite maximum samples'):
        Engine.ensemble_sweep(engines, 'mes', np.array([1.0, np.nan, 2.0]), p['Z'])
    with pytest.raises(GpxError, match='mixture moments are only formed for UCB / mean') as err:
        Engine.ensemble_sweep(engines, 'mes', np.ones(3), p['Z'], want_moments=True)
    assert err.value.code == GPX_EARG
    ok = Engine.ensemble_sweep(engines, 'mes', np.full((3, 64), 2.0), p['Z'])['acq']       # S = 64 per member is allowed
    assert np.isfinite(ok).all()
    for e in engines:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from pybo_amd._lib import Engine, GpxError, GPX_EARG
    p = _problem()
    mu, s2 = _mean('se')
    e = _fitted('se')
    good = p['ys'][7]
    want = e.sweep('mes', good, p['Z'])['acq']
    finite = 'MES takes 1 to 64 finite maximum samples'
    for bad in (np.zeros(0), np.ones(65), np.array([1.0, np.nan]), np.array([np.inf]), np.array([1.0, -np.inf, 2.0])):
        with pytest.raises(GpxError, match='sweep: ' + finite) as err:
            e.sweep('mes', bad, p['Z'])
        assert err.value.code == GPX_EARG
        assert np.array_equal(e.sweep('mes', good, p['Z'])['acq'], want)
    for aid in (4, 15, 17):                                     # only 16 is MES
        with pytest.raises(GpxError, match='sweep: unknown acquisition id'):
            e.sweep(aid, good, p['Z'])
    e.set_option('sweep_cache', 1)
    e.sweep('mes', good, p['Z'], k=1)
    e.set_option('sweep_cache', 0)
    with pytest.raises(GpxError, match='sweep_update: ' + finite):
        e.sweep_update('mes', np.ones(65), k=1)
    with pytest.raises(GpxError, match='sweep_batch: MES is not supported') as err:
        e.sweep_batch('mes', good, 2)
    assert err.value.code == GPX_EARG
    with pytest.raises(GpxError, match='ensemble_sweep_batch: MES is not supported') as err:
        Engine.ensemble_batch([e], 'mes', good, 2)
    assert err.value.code == GPX_EARG
    assert np.array_equal(e.sweep_update('mes', good)['acq'], want)
    assert e.sweep_batch('ei', 0.5, 2)['sel_idx'].shape == (2,)          # the cache a MES sweep seeded serves the batch entry
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# no pruning
# ---------------------------------------------------------------------------------------------------------------------
def test_mes_never_prunes_and_leaves_the_hint_alone():
    """prune = 1, selection-only, M = 65536, N = 1024 (tests/test_gpu_prune_hint.py's model, f = 0.5): the MES call runs the plain loop
    and an EI sweep before and after prunes.  Under prune = -1 the carried decision is neither read, armed nor dropped by a MES call:
    sweep_core touches it only inside the pruning branch, which MES never enters -- so the EI sweep after it skips its gate exactly
    when the EI sweep before it earned that."""
    from test_gpu_prune import _dev
    rng = np.random.RandomState(2)
    n, d, m, k = 1024, 8, 65536, 10
    X = rng.rand(n, d)
    y = -np.sum((X - 0.5) ** 2, axis=1) + 1e-3 * rng.randn(n)
    rho, bias = float(np.var(y)), float(np.mean(y))
    Z = np.random.RandomState(5).rand(m, d)
    dZ = _dev(Z)
    e = _engine()
    e.fit(X, y, 'se', 0.5 * np.ones(d), rho, 1e-4 * rho, bias)
    target = e.mean_at_obs()[1]
    ys = target + 0.05 * np.sqrt(rho) * (1.0 + np.arange(7))
    e.set_option('prune', 1)
    ei0 = e.sweep_dev('ei', target, dZ.data_ptr(), m, k)
    assert e.prune_report(vectors=False)['path'] == 'pruned'
    e.timers(reset=True)
    top = e.sweep_dev('mes', ys, dZ.data_ptr(), m, k)
    t = e.timers(reset=True)
    r = e.prune_report(vectors=False)
    assert r['path'] == 'plain' and t['sweep_bound'] == 0.0
    assert t['sweep_trmm_flop'] == float(n) ** 2 * m            # every candidate, exactly
    ei1 = e.sweep_dev('ei', target, dZ.data_ptr(), m, k)
    assert e.prune_report(vectors=False)['path'] == 'pruned'
    assert np.array_equal(ei0[0], ei1[0]) and np.array_equal(ei0[1], ei1[1])
    # the plain loop's values: the call that returns every value
    full = e.sweep('mes', ys, Z, k=k)
    assert np.array_equal(top[0], full['top_val']) and np.array_equal(top[1], full['top_idx'])
    assert np.array_equal(top[1], gp_ref.topk_desc(full['acq'], k))
    # the carried decision
    e.set_option('prune', -1)
    a = e.sweep_dev('ei', target, dZ.data_ptr(), m, k)
    ra = e.prune_report(vectors=False)
    e.sweep_dev('mes', ys, dZ.data_ptr(), m, k)
    assert e.prune_report(vectors=False)['path'] == 'plain'
    b = e.sweep_dev('ei', target, dZ.data_ptr(), m, k)
    rb = e.prune_report(vectors=False)
    earned = ra['path'] == 'pruned' and ra['nsurv'] <= ra['cap'] // 2
    assert not ra['gate_hint'] and rb['gate_hint'] == earned, (ra, rb)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], ei0[1])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# plug-in level
# ---------------------------------------------------------------------------------------------------------------------
def test_the_policy_on_device_models():
    from pybo_amd import models, policies, solvers
    from pybo_amd._lib import DeviceGrid
    p = _problem()
    bounds = np.array([[0.0, 1.0]] * D)
    X, y = p['X'][:N], p['y'][:N]
    gp = models.make_gp(SN2, RHO, p['ell'], BIAS)
    gp.add_data(X, y)
    index = policies.MES(gp, bounds, X, nmax=7, ngrid=2000, rng=3)
    kind, ystar = index.acq
    assert kind == 'mes' and ystar.shape == (7,) and hasattr(index, 'topk') and not hasattr(index, 'batch')
    # the index is the device sweep; the closure on the moments a 'mean' sweep of the same handle returns bounds it
    Z = p['Z'][:200]
    vals = index(Z)
    eng = index.topk_engine()
    m = eng.sweep('mean', None, Z, want_moments=True)
    _within(m['mu'], m['s2'], ystar, vals, np.arange(0, 200, 10))
    # with grad: the closure and its chain rule on the moments and gradients predict(grad=True) returns
    from pybo_amd.mes import mes_value_grad
    f, G = index(Z[:6], grad=True)
    fw, Gw = mes_value_grad(*eng.predict(Z[:6], grad=True), ystar)
    assert G.shape == (6, D) and np.array_equal(f, fw) and np.array_equal(G, Gw) and np.isfinite(G).all()
    assert np.all(np.abs(f - vals[:6]) <= 1e-5 * vals[:6])        # (the two paths' moments agree to the stated 1e-6)
    # solve_lbfgs over a resident grid: .topk (a cold sweep that seeds the cache), then the warm re-score
    grid = DeviceGrid('uniform', bounds, 4097, seed=5)
    eng.timers(reset=True)
    v1, i1 = index.topk(grid, 3)
    t1 = eng.timers(reset=True)
    v2, i2 = index.topk(grid, 3)
    t2 = eng.timers(reset=True)
    assert t1['sweep_trmm_launches'] >= 1 and t2['sweep_trmm_launches'] == 0
    assert np.array_equal(v1, v2) and np.array_equal(i1, i2)
    x, fx = solvers.solve_lbfgs(index, bounds, nbest=3, xgrid=grid)
    assert np.all((x >= 0) & (x <= 1)) and fx >= v1[0] * (1 - 1e-9)
    xb, fb = solvers.solve_lbfgs(index, bounds, nbest=3, xgrid=grid, select='best')
    assert np.all((xb >= 0) & (xb <= 1)) and fb >= fx * (1 - 1e-9)
    grid.close()
    # an ensemble over three device members: one set of maxima per member, the ensemble sweep behind index and topk
    small = models.make_gp(1e-3, 1.0, [0.4, 0.4, 0.4], 0.0)
    small.params['like.sn2'].set_prior('horseshoe', 0.1)
    small.params['kern.rho'].set_prior('lognormal', 0.0, 1.0)
    small.params['kern.ell'].set_prior('uniform', [0.02] * D, [3.0] * D)
    small.params['mean.bias'].set_prior('normal', 0.0, 4.0)
    small.add_data(X[:40], y[:40])
    ens = models.MCMC(small, n=3, burn=10, rng=7)
    eidx = policies.MES(ens, bounds, X[:40], nmax=4, ngrid=500, rng=1)
    ys = eidx.acq[1]
    assert ys.shape == (3, 4)
    ev = eidx(Z)
    singles = [m._engine().sweep('mes', ys[j], Z)['acq'] for j, m in enumerate(ens.members)]
    assert np.array_equal(ev, ((singles[0] + singles[1]) + singles[2]) / 3.0)
    tv, ti = eidx.topk(Z, 5)
    assert np.array_equal(ti, gp_ref.topk_desc(ev, 5)) and np.array_equal(tv, ev[ti])
    fe, Ge = eidx(Z[:4], grad=True)
    assert Ge.shape == (4, D) and np.isfinite(Ge).all() and np.all(np.abs(fe - ev[:4]) <= 1e-5 * ev[:4])
