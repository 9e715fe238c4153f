"""The knowledge gradient on the device (GPX_ACQ_KG = 32, gpx_kg_grad: pybo_amd/csrc/kernels_kg.hip, kg_math.h) against the oracle of
tests/kg_ref.py -- fp64 numpy GP algebra and the 50-digit envelope -- on EVERY candidate, through every entry that takes it, and
what refuses it.  Every test here fails on a library that refuses id 32.

Shapes, the smallest at which the kernels can go wrong: N = 130 and 200 (Np = 256: two row blocks, the second ragged) and 128 (an
exact block); M = 300 (three panels, the last with 44 columns; five workgroups of k_acq_kg, the last with 44 candidates); d = 1, 3, 33;
all four covariances; m = 1, 2, 63, 64, 127 support points.

Tolerance of a value (kg_ref.value_tol), from the stated moment tolerances of tests/helpers.py and no new
number: 2 max_j |d alpha_j| + 0.8 max_j |d beta_j|.  The inputs are chosen so that the oracle alone shows at least 20 % of the
candidates at or above 1e-3 of the largest value in every case, and in the all-negative-means cases (bias = -2) that a padding column
taken for a line (0, 0) would move at least 10 % of the values."""
import numpy as np
import pytest

import kg_ref
from oracle import gp_ref
from helpers import synth_problem, s2_tol, mu_tol

pytestmark = pytest.mark.gpu

M = 300
RHO, SN2 = 1.3, 1e-2
# kernel, N, d, m, ell, bias (< 0: the targets are shifted by it too, every posterior mean is negative)
CASES = {
    'se_neg_m63': ('se', 200, 3, 63, 0.15, -2.0),
    'se_m127': ('se', 200, 3, 127, 0.15, 0.2),
    'matern5_m64': ('matern5', 130, 3, 64, 0.3, 0.2),
    'matern3_d1_m2': ('matern3', 128, 1, 2, 0.1, 0.2),
    'matern1_d33_m1': ('matern1', 200, 33, 1, 2.0, 0.2),
    'matern1_neg_m63': ('matern1', 130, 3, 63, 0.3, -2.0),
    'matern5_d33_m127': ('matern5', 200, 33, 127, 2.0, 0.2),
}
_CACHE = {}


def _engine():
    from pybo_amd._lib import Engine
    return Engine(0)


def _case(name):
    """The problem, the oracle's lines and the 50-digit values of a case: computed once, shared, never written to."""
    if name not in _CACHE:
        kernel, N, d, m, ell, bias = CASES[name]
        X, y, _ = synth_problem(N, d, seed=3)
        y = y + min(bias, 0.0)
        rng = np.random.RandomState(5)
        Z, A = rng.rand(M, d), rng.rand(m, d)
        ell = np.full(d, ell)
        model = kg_ref.make_model(X, y, kernel, ell, RHO, SN2, bias)
        want, alpha, beta = kg_ref.kg_oracle(model, A, Z)
        for v in (X, y, Z, A, want, alpha, beta):
            v.setflags(write=False)
        _CACHE[name] = dict(kernel=kernel, X=X, y=y, ell=ell, bias=bias, Z=Z, A=A, model=model, want=want, alpha=alpha, beta=beta,
                            tol=kg_ref.value_tol(model, alpha, beta, RHO))
    return _CACHE[name]


def _fitted(c):
    e = _engine()
    e.fit(c['X'], c['y'], c['kernel'], c['ell'], RHO, SN2, c['bias'])
    return e


# ---------------------------------------------------------------------------------------------------------------------
# 1. values against the oracle on every candidate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_values_moments_and_topk_against_the_oracle(name):
    from pybo_amd.kg import kg_value
    c = _case(name)
    want, tol = c['want'], c['tol']
    # what the oracle alone shows about the inputs
    assert np.mean(want >= 1e-3 * want.max()) >= 0.2
    if c['bias'] < 0:
        assert c['alpha'].max() < 0.0
        padded = kg_value(*kg_ref.add_padding_line(c['alpha'], c['beta']))
        assert np.mean(np.abs(padded - want) > 1e-3 * want.max()) >= 0.1
    e = _fitted(c)
    r = e.sweep('kg', c['A'], c['Z'], k=10, want_moments=True)
    got = r['acq']
    err = np.abs(got - want)
    print('%s: max error %.3g, max error / tolerance %.3g' % (name, err.max(), (err / tol).max()))
    assert np.isfinite(got).all() and np.all(got >= 0.0) and not np.signbit(got).any()
    assert np.all(err <= tol), (np.argmax(err / tol), (err / tol).max())              # every candidate, none left out
    mu, s2 = c['model'].predict(c['Z'])
    assert np.all(np.abs(r['mu'] - mu) <= mu_tol(mu, RHO)) and np.all(np.abs(r['s2'] - s2) <= s2_tol(s2, RHO))
    idx = gp_ref.topk_desc(got, 10)
    assert np.array_equal(r['top_idx'], idx) and np.array_equal(r['top_val'], got[idx])
    for k in (1, 64):
        t = e.sweep('kg', c['A'], c['Z'], k=k, want_all=False)               # the selection-only call: never pruned, the same values
        idx = gp_ref.topk_desc(got, k)
        assert np.array_equal(t['top_idx'], idx) and np.array_equal(t['top_val'], got[idx])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. layout independence, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['se_m127', 'matern5_m64', 'matern1_d33_m1'])
def test_a_value_depends_on_the_candidate_and_the_support_set_alone(name):
    from test_gpu_prune import _DevBuf, _dev
    c = _case(name)
    Z, A = c['Z'], c['A']
    e = _fitted(c)
    host = e.sweep('kg', A, Z, k=7, want_moments=True)
    vals = host['acq']
    # gpx_sweep against gpx_sweep_dev
    dZ, buf, bmu, bs2 = _dev(Z), _DevBuf(M), _DevBuf(M), _DevBuf(M)
    tv, ti = e.sweep_dev('kg', A, dZ.data_ptr(), M, 7, d_acq=buf.data_ptr(), d_mu=bmu.data_ptr(), d_s2=bs2.data_ptr())
    e.sync()
    assert np.array_equal(buf.numpy(), vals) and np.array_equal(tv, host['top_val']) and np.array_equal(ti, host['top_idx'])
    assert np.array_equal(bmu.numpy(), host['mu']) and np.array_equal(bs2.numpy(), host['s2'])
    # candidates permuted; the same candidate in different panels and lanes
    perm = np.random.RandomState(1).permutation(M)
    assert np.array_equal(e.sweep('kg', A, Z[perm])['acq'], vals[perm])
    Zr = Z.copy()
    where = [0, 63, 64, 127, 128, 200, 256, 299]
    Zr[where] = Z[17]
    rep = e.sweep('kg', A, Zr)['acq']
    assert np.all(rep[where] == vals[17]) and np.array_equal(np.delete(rep, where), np.delete(vals, where))
    # a shorter candidate array (other block and panel boundaries)
    assert np.array_equal(e.sweep('kg', A, Z[3:132])['acq'], vals[3:132])
    # option chunk = 128 against the default: three chunks of one panel
    e.set_option('chunk', 128)
    small = e.sweep('kg', A, Z, k=7, want_moments=True)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        assert np.array_equal(small[key], host[key]), key
    # support rows permuted: another summation order of the product and of the lines, within the oracle tolerance only
    sp = np.random.RandomState(2).permutation(len(A))
    other = e.sweep('kg', A[sp], Z)['acq']
    assert np.all(np.abs(other - c['want']) <= c['tol'])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. degenerate inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['se_m127', 'matern1_neg_m63'])
def test_degenerate_inputs_stay_finite_and_within_tolerance(name):
    c = _case(name)
    A = c['A'].copy()
    A[5] = A[4]                                   # two identical support points
    Z = c['Z'][:40].copy()
    Z[0] = A[3]                                   # a candidate equal to a support point
    Z[1] = A[4]                                   # ... to the duplicated one
    Z[2] = c['X'][0]                              # a candidate equal to an observed point
    Z[3] = c['X'][7]
    e = _fitted(c)
    for sup in (A, A[:1], A[4:6]):                # the whole set, m = 1, and the duplicated pair alone
        want, alpha, beta = kg_ref.kg_oracle(c['model'], sup, Z)
        tol = kg_ref.value_tol(c['model'], alpha, beta, RHO)
        got = e.sweep('kg', sup, Z)['acq']
        assert np.isfinite(got).all() and np.all(got >= 0.0)
        assert np.all(np.abs(got - want) <= tol), (len(sup), np.abs(got - want) / tol)
    # the candidate on the only support point: two nearly identical lines, the value is what one observation teaches about that point
    one = e.sweep('kg', A[3:4], Z[:1])['acq']
    want, alpha, beta = kg_ref.kg_oracle(c['model'], A[3:4], Z[:1])
    assert np.isfinite(one).all() and abs(one[0] - want[0]) <= kg_ref.value_tol(c['model'], alpha, beta, RHO)[0]
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. moments and cache
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['se_neg_m63', 'matern5_m64'])           # (N = 200, 130: an append stays inside the second block)
def test_moments_are_an_ei_sweeps_and_a_kg_sweep_seeds_the_cache_as_ei_does(name):
    c = _case(name)
    Z, A = c['Z'], c['A']
    target = float(c['y'].max())
    e, f = _fitted(c), _fitted(c)
    e.set_option('sweep_cache', 1)
    f.set_option('sweep_cache', 1)
    kg = e.sweep('kg', A, Z, k=3, want_moments=True)
    ei = f.sweep('ei', target, Z, k=3, want_moments=True)
    e.set_option('sweep_cache', 0)
    f.set_option('sweep_cache', 0)
    assert np.array_equal(kg['mu'], ei['mu']) and np.array_equal(kg['s2'], ei['s2'])
    assert e.sweep_cache_size() == f.sweep_cache_size() == M
    a, b = e.sweep_update('ei', target, k=5, want_moments=True), f.sweep_update('ei', target, k=5, want_moments=True)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a['acq'], ei['acq'])
    ba, bb = e.sweep_batch('ei', target, 4), f.sweep_batch('ei', target, 4)
    for key in ('sel_val', 'sel_idx', 'sel_s2'):
        assert np.array_equal(ba[key], bb[key]), key
    # after an append the two caches still agree, and a cold KG sweep without the option leaves the cache alone
    x_new, y_new = np.full(Z.shape[1], 0.37), 0.1 + min(c['bias'], 0.0)
    assert e.append(x_new, y_new) and f.append(x_new, y_new)
    again = e.sweep('kg', A, Z[:50])['acq']
    assert np.isfinite(again).all() and e.sweep_cache_size() == M
    a, b = e.sweep_update('ei', target, k=5), f.sweep_update('ei', target, k=5)
    for key in ('acq', 'top_val', 'top_idx'):
        assert np.array_equal(a[key], b[key]), key
    e.close()
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. gpx_kg_grad
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_value_and_gradient_at_points(name):
    c = _case(name)
    Z, A = c['Z'], c['A']
    e = _fitted(c)
    rows = np.r_[0:5, 126:131, 295:300]
    vals = e.sweep('kg', A, Z)['acq']
    f, g = e.kg_grad(A, Z[rows])
    assert f.shape == (15,) and g.shape == (15, Z.shape[1]) and np.isfinite(g).all()
    assert np.all(np.abs(f - vals[rows]) <= c['tol'][rows])
    fw, gw = kg_ref.kg_oracle_grad(c['model'], A, Z[rows])
    assert np.all(np.abs(f - fw) <= c['tol'][rows])
    np.testing.assert_allclose(g, gw, rtol=1e-6, atol=1e-8)
    assert np.abs(gw).max() > 1e-3
    # a row does not depend on the batch it travels in: M = 1 and M = 5, and the whole array (three panels of points)
    f5, g5 = e.kg_grad(A, Z[:5])
    f1, g1 = e.kg_grad(A, Z[:1])
    assert np.array_equal(f5, f[:5]) and np.array_equal(g5, g[:5]) and np.array_equal(f1, f[:1]) and np.array_equal(g1, g[:1])
    fa, ga = e.kg_grad(A, Z)
    assert np.array_equal(fa[rows], f) and np.array_equal(ga[rows], g)
    # fit, cache and queue untouched: the sweep after it returns the bits of the sweep before it
    assert np.array_equal(e.sweep('kg', A, Z)['acq'], vals)
    e.close()


def test_kg_grad_refuses_bad_arguments():
    from pybo_amd._lib import GpxError, GPX_EARG, GPX_ESTATE
    c = _case('matern5_m64')
    e = _engine()
    A2, Z1, f0, g0 = np.ascontiguousarray(c['A'][:2]), np.ascontiguousarray(c['Z'][:1]), np.empty(1), np.empty(3)
    with pytest.raises(GpxError, match='kg_grad: model is not fitted') as err:
        e._check(e._lib.gpx_kg_grad(e._h, A2.ctypes.data, 2, Z1.ctypes.data, 1, f0.ctypes.data, g0.ctypes.data))
    assert err.value.code == GPX_ESTATE
    e.close()
    e = _fitted(c)
    bad_nan = c['A'].copy()
    bad_nan[2, 1] = np.nan
    for bad in (np.zeros((128, 3)), bad_nan):
        with pytest.raises(GpxError, match=r'kg_grad: KG takes m \* d finite support coordinates, m in \[1, 127\]') as err:
            e.kg_grad(bad, c['Z'][:2])
        assert err.value.code == GPX_EARG
    with pytest.raises(GpxError, match=r'kg_grad: M must be in \[1, 4096\]'):
        e.kg_grad(c['A'], np.zeros((4097, 3)))
    f, g = e.kg_grad(c['A'], c['Z'][:2])
    assert np.isfinite(f).all() and np.isfinite(g).all()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_handle_cache_and_announcement_as_they_were():
    from pybo_amd._lib import Engine, GpxError, GPX_EARG
    from test_gpu_prune import _dev
    c = _case('matern5_m64')
    Z, A = c['Z'], c['A']
    d = Z.shape[1]
    e, twin = _fitted(c), _fitted(c)
    want = e.sweep('kg', A, Z)['acq']
    takes = r'sweep: KG takes m \* d finite support coordinates, m in \[1, 127\]'
    nan, inf = A.copy(), A.copy()
    nan[7, 0], inf[0, 2] = np.nan, -np.inf
    dZ = _dev(Z)
    for bad in (np.zeros(0), np.ones(d + 1), np.ones(128 * d), nan, inf):        # m = 0, not a multiple of d, m = 128, NaN, inf
        for call in (lambda: e.sweep('kg', bad, Z), lambda: e.sweep_dev('kg', bad, dZ.data_ptr(), M, 3)):
            with pytest.raises(GpxError, match=takes) as err:
                call()
            assert err.value.code == GPX_EARG
    assert np.array_equal(e.sweep('kg', A, Z)['acq'], want)
    for aid in list(range(17, 32)) + [4, 15, 33]:                                # only 32 is KG
        with pytest.raises(GpxError, match='sweep: unknown acquisition id'):
            e.sweep(aid, A, Z)
    # a live cache, a queued correction and a pending announcement
    target = float(c['y'].max())
    for eng in (e, twin):
        eng.set_option('sweep_cache', 1)
        eng.sweep('ei', target, Z, k=1)
        eng.set_option('sweep_cache', 0)
        assert eng.append(np.full(d, 0.41), 0.3)
        assert eng.append_begin(np.full(d, 0.62))
    for entry, call in (('sweep_update', lambda: e.sweep_update('kg', A, k=1)),
                        ('sweep_batch', lambda: e.sweep_batch('kg', A, 2)),
                        ('ensemble_sweep', lambda: Engine.ensemble_sweep([e], 'kg', A, Z)),
                        ('ensemble_sweep', lambda: Engine.ensemble_sweep([e, twin], 'kg', A, Z, k=2)),
                        ('ensemble_sweep_batch', lambda: Engine.ensemble_batch([e], 'kg', A, 2))):
        with pytest.raises(GpxError, match='%s: KG is not supported' % entry) as err:
            call()
        assert err.value.code == GPX_EARG
    with pytest.raises(GpxError, match='sweep_update: KG is not supported'):
        tv, ti = np.empty(1), np.empty(1, dtype=np.int64)
        p = np.ascontiguousarray(A).reshape(-1)
        e._check(e._lib.gpx_sweep_update_dev(e._h, 32, p.ctypes.data, len(p), 1, tv.ctypes.data, ti.ctypes.data, None, None, None))
    assert e.sweep_cache_size() == twin.sweep_cache_size() == M
    for eng in (e, twin):
        assert eng.append(np.full(d, 0.62), -0.2)                                # the announced point: consumed by both alike
    a, b = e.sweep_update('ei', target, k=5, want_moments=True), twin.sweep_update('ei', target, k=5, want_moments=True)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        assert np.array_equal(a[key], b[key]), key
    e.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. plug-in level
# ---------------------------------------------------------------------------------------------------------------------
def test_policy_solver_and_loop_on_device_models():
    import pybo_amd
    from pybo_amd import models, policies, solvers
    from pybo_amd._lib import DeviceGrid
    c = _case('matern5_m64')
    d = 3
    bounds = np.array([[0.0, 1.0]] * d)
    X, y = c['X'], c['y']
    gp = models.make_gp(SN2, RHO, c['ell'], c['bias'], kernel='matern5')
    gp.add_data(X, y)
    index = policies.KG(gp, bounds, X, nsupport=20, ngrid=500, rng=3)
    kind, support = index.acq
    assert kind == 'kg' and support.shape == (20, d) and hasattr(index, 'topk') and not hasattr(index, 'batch')
    mu = gp.predict_mean(support)
    assert np.all(np.diff(mu) <= 0.0)                                # the support set: posterior mean descending
    # the index against the oracle on its own support set
    Z = c['Z'][:100]
    vals = index(Z)
    want, alpha, beta = kg_ref.kg_oracle(c['model'], support, Z)
    assert np.all(np.abs(vals - want) <= kg_ref.value_tol(c['model'], alpha, beta, RHO))
    f, G = index(Z[:4], grad=True)
    assert G.shape == (4, d) and np.all(np.abs(f - vals[:4]) <= 1e-9 + 1e-6 * vals[:4])
    # solve_lbfgs with a host grid and with a resident one; a resident grid is swept cold every time and no cache is left behind
    xg = np.random.RandomState(4).rand(1000, d)
    x, fx = solvers.solve_lbfgs(index, bounds, nbest=3, xgrid=xg)
    tv, ti = index.topk(xg, 3)
    assert np.all((x >= 0) & (x <= 1)) and fx >= tv[0] * (1 - 1e-9)
    grid = DeviceGrid('uniform', bounds, 1025, seed=5)
    eng = index.topk_engine()
    eng.timers(reset=True)
    v1, i1 = index.topk(grid, 3)
    v2, i2 = index.topk(grid, 3)
    t = eng.timers(reset=True)
    assert t['sweep_trmm_launches'] == 2 and eng.sweep_cache_size() == 0
    assert np.array_equal(v1, v2) and np.array_equal(i1, i2)
    assert np.array_equal(v1, index(np.asarray(grid)[i1]))
    xd, fd = solvers.solve_lbfgs(index, bounds, nbest=3, xgrid=grid)
    assert np.all((xd >= 0) & (xd <= 1)) and fd >= v1[0] * (1 - 1e-9)
    # a live cache of another policy is neither used nor touched by KG's top-k
    geng = gp._engine()
    target = float(y.max())
    ev, ei_i = gp.acq_topk('ei', target, grid, 3)                   # seeds gp's cache with the grid
    assert geng.sweep_cache_size() == len(grid)
    geng.timers(reset=True)
    kv, ki = gp.acq_topk('kg', support, grid, 3)                    # cold, although a matching cache is live
    t = geng.timers(reset=True)
    assert t['sweep_trmm_launches'] == 1 and geng.sweep_cache_size() == len(grid)
    assert np.array_equal(kv, v1) and np.array_equal(ki, i1)
    ev2, ei_i2 = gp.acq_topk('ei', target, grid, 3)                 # ... which still serves the warm re-score
    t = geng.timers(reset=True)
    assert t['sweep_trmm_launches'] == 0 and np.array_equal(ev, ev2) and np.array_equal(ei_i, ei_i2)
    grid.close()
    # the loop
    obj = lambda x: float(-np.sum((np.ravel(x) - 0.4) ** 2))
    small = models.make_gp(1e-2, 1.0, [0.4] * d, 0.0)
    out = pybo_amd.solve_bayesopt(obj, bounds, model=small, niter=5, policy=('kg', {'nsupport': 8, 'ngrid': 200}),
                                  solver=('lbfgs', {'nbest': 2, 'ngrid': 200}), rng=1)
    assert np.all(np.isfinite(np.ravel(out[0])))
    # the ensemble: the member-order mean of the members' sweeps, no .topk; the loop on it
    proto = models.make_gp(1e-2, 1.0, [0.4] * d, 0.0)
    proto.params['like.sn2'].set_prior('horseshoe', 0.1)
    proto.params['kern.rho'].set_prior('lognormal', 0.0, 1.0)
    proto.params['kern.ell'].set_prior('uniform', [0.02] * d, [3.0] * d)
    proto.params['mean.bias'].set_prior('normal', 0.0, 4.0)
    proto.add_data(X[:40], y[:40])
    ens = models.MCMC(proto, n=3, burn=10, rng=7)
    eidx = policies.KG(ens, bounds, X[:40], nsupport=6, ngrid=100, rng=1)
    assert eidx.acq[0] == 'kg' and not hasattr(eidx, 'topk') and not hasattr(eidx, 'batch')
    sup = eidx.acq[1]
    ev = eidx(Z)
    singles = [m._engine().sweep('kg', sup, Z)['acq'] for m in ens.members]
    assert np.array_equal(ev, ((singles[0] + singles[1]) + singles[2]) / 3.0)
    fe, Ge = eidx(Z[:3], grad=True)
    assert Ge.shape == (3, d) and np.isfinite(Ge).all() and np.all(np.abs(fe - ev[:3]) <= 1e-9 + 1e-6 * ev[:3])
    out = pybo_amd.solve_bayesopt(obj, bounds, model=ens, niter=5, policy='kg', solver=('lbfgs', {'nbest': 2, 'ngrid': 100}), rng=1)
    assert np.all(np.isfinite(np.ravel(out[0]))) and out[1].ndata == 40 + 6
