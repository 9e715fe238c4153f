"""Two-objective sweeps on the device: gpx_ehvi_sweep[_dev] and gpx_ehvi_fold_dev return the expected
hypervolume improvement of two independent posteriors over a Pareto front.  Bit for bit: the empty front against the members' own EI
sweeps, the sweep against the fold alone on the sweep's moments, host against device form, permuted and sub-range candidates.  To
1e-9 S + TINY: the kernel alone against pareto.ehvi_from_moments (scipy's erfc; erfcx below z = -6, where the plain form of EI has lost its
digits by z = -38) on the same moment bits, S the magnitude sum of ehvi_ref.py.
End to end: against the oracle at the stated moment tolerances propagated through the closed form.  Shapes: ehvi_cases.py.

Measured on an MI355X, the kernel alone over its twelve cases: largest error / S 3.02e-10 (n = 1024, M = 13001; z = -38), allowed 1e-9
(profiles/ehvi_sweep.md); end to end the worst error is 8.4e-08 of its tolerance."""
import ctypes as C

import numpy as np
import pytest

from oracle import gp_ref
import ehvi_cases as cases
import ehvi_ref
from test_gpu_prune import _dev, _DevBuf
from test_gpu_ens_prune import _dev_cand, _same, _topk_of

pytestmark = pytest.mark.gpu


def _fit_engines(p, n=None):
    from pybo_amd._lib import Engine
    n = len(p['X']) if n is None else n
    engines = []
    for j, (sn2, rho, ell, bias) in enumerate(p['hypers']):
        e = Engine(0)
        e.fit(p['X'][:n], p['Y'][:n, j], p['kernels'][j], ell, rho, sn2, bias)
        engines.append(e)
    return engines


_CASE = {}


def _case(name):
    """The case's problem and its two fitted engines, once per session."""
    if name not in _CASE:
        p = cases.problem(name)
        _CASE[name] = (p, _fit_engines(p))
    p, engines = _CASE[name]
    for e in engines:
        e.set_option('sweep_cache', -1)
    return p, engines


def _bits(a, b):
    """bit for bit; any NaN equals any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def _data_front(p):
    """The observations themselves as the raw front (dominated points included) and the policy's reference point for them."""
    from pybo_amd import pareto
    return p['Y'], pareto.default_ref(p['Y'])


# ---- 1. empty front ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_empty_front_is_the_product_of_the_members_own_ei_sweeps(name):
    from pybo_amd._lib import Engine
    p, (f1, f2) = _case(name)
    Z, M = p['Z'], len(p['Z'])
    ref = np.array([np.median(p['Y'][:, 0]), np.median(p['Y'][:, 1])])
    e1 = f1.sweep('ei', ref[0], Z, k=0)['acq']
    e2 = f2.sweep('ei', ref[1], Z, k=0)['acq']
    want = np.where(e1 < 0, 0.0, e1) * e2 + 0.0
    assert want.max() > 1e-4 and (want > 0).sum() > M // 2
    got = Engine.ehvi_sweep(f1, f2, None, ref, Z, k=10, want_all=True)
    assert _bits(got['acq'], want)
    assert _same((got['top_val'], got['top_idx']), _topk_of(want, 10))
    # raw points that all lie on or below the reference point are an empty front too
    below = np.array([[ref[0], ref[1] + 1.0], [ref[0] - 1.0, ref[1] - 1.0], [ref[0] + 1.0, ref[1]]])
    assert _bits(Engine.ehvi_sweep(f1, f2, below, ref, Z, k=0, want_all=True)['acq'], want)
    dacq = _DevBuf(M)
    d = Engine.ehvi_sweep(f1, f2, None, ref, _dev_cand(Z), k=10, d_acq=dacq.data_ptr())
    assert _bits(dacq.numpy(), want) and _same((d['top_val'], d['top_idx']), (got['top_val'], got['top_idx']))


# ---- 2. sweep against fold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_the_sweep_is_the_fold_of_the_members_own_moments(name):
    from pybo_amd._lib import Engine
    p, (f1, f2) = _case(name)
    Z, M, k = p['Z'], len(p['Z']), 10
    P, ref = _data_front(p)
    assert len(ehvi_ref.strips(P, ref)[1]) - 1 >= 5
    dZ = _dev_cand(Z)
    dacq, dmom = _DevBuf(M), _DevBuf(4 * M)
    r = Engine.ehvi_sweep(f1, f2, P, ref, dZ, k=k, d_acq=dacq.data_ptr(), d_mom=dmom.data_ptr())
    vals, mom = dacq.numpy(), dmom.numpy().reshape(4, M)
    assert _same((r['top_val'], r['top_idx']), _topk_of(vals, k)) and vals.max() > 0
    # d_mom holds each member's own gpx_sweep_dev moments
    for j, f in enumerate((f1, f2)):
        dmu, ds2 = _DevBuf(M), _DevBuf(M)
        f.sweep_dev('mean', None, dZ.ptr, M, 0, d_mu=dmu.data_ptr(), d_s2=ds2.data_ptr())
        f.sync()
        assert _bits(mom[2 * j], dmu.numpy()) and _bits(mom[2 * j + 1], ds2.numpy())
    # the fold alone on those moments: the sweep's values and top-k, led by either handle
    for lead in (f1, f2):
        dout = _DevBuf(M)
        g = lead.ehvi_fold(dmom.data_ptr(), M, P, ref, k=k, d_acq=dout.data_ptr())
        assert _bits(dout.numpy(), vals) and _same((g['top_val'], g['top_idx']), (r['top_val'], r['top_idx']))
    # no vector asked for, and the host form
    none = Engine.ehvi_sweep(f1, f2, P, ref, dZ, k=k)
    assert _same((none['top_val'], none['top_idx']), (r['top_val'], r['top_idx']))
    host = Engine.ehvi_sweep(f1, f2, P, ref, Z, k=k, want_all=True)
    assert _bits(host['acq'], vals) and _same((host['top_val'], host['top_idx']), (r['top_val'], r['top_idx']))
    only = Engine.ehvi_sweep(f1, f2, P, ref, Z, k=k, want_all=False)
    assert only['acq'] is None and _same((only['top_val'], only['top_idx']), (r['top_val'], r['top_idx']))
    # a live sweep cache on a member is re-seeded as its own gpx_sweep_dev would
    f2.set_option('sweep_cache', 1)
    cached = Engine.ehvi_sweep(f1, f2, P, ref, Z, k=k, want_all=True)
    assert _bits(cached['acq'], vals) and f2.sweep_cache_size() == M and f1.sweep_cache_size() == 0
    assert _bits(f2.sweep_update('mean', None, k=0, want_all=True)['acq'], mom[2])
    f2.set_option('sweep_cache', -1)


# ---- 3. the kernel alone -------------------------------------------------------------------------------------------------------
_FRONTS = {}


def _front(n):
    if n not in _FRONTS:
        from pybo_amd import pareto
        P, ref = cases.raw_front(n, seed=40 + n)
        a, b = pareto.strips(P, ref)
        assert len(b) - 1 == n and len(P) > n
        _FRONTS[n] = (P, ref, a, b)
    return _FRONTS[n]


def _magnitude(mom, a, b):
    return np.concatenate([ehvi_ref.magnitude(*mom[:, i:i + 1024], a, b) for i in range(0, mom.shape[1], 1024)])


@pytest.mark.parametrize('M', [1, 257, 13001])
@pytest.mark.parametrize('n', [1, 7, 64, 1024])
def test_the_fold_kernel_against_the_closed_form_on_the_same_moments(n, M):
    """Moments with z from -40 to +40 on both objectives, variances down to the floor, a NaN and a +inf mean.  Where S is not finite (the
    +inf mean: every EI_2 is +inf, and w_i * inf is NaN for a w_i of exactly 0) both sides must be non-finite; a NaN moment gives NaN."""
    from pybo_amd import pareto
    from pybo_amd._lib import Engine
    P, ref, a, b = _front(n)
    mom = cases.synthetic_moments(M, seed=7 * n + M)
    lead = Engine(0)
    k = min(M, 10)
    dmom, dout = _dev(mom), _DevBuf(M)
    r = lead.ehvi_fold(dmom.data_ptr(), M, P, ref, k=k, d_acq=dout.data_ptr())
    got = dout.numpy()
    want = pareto.ehvi_from_moments(*mom, a, b)
    S = _magnitude(mom, a, b)
    fin = np.isfinite(S)
    err = np.abs(got[fin] - want[fin])
    tol = 1e-9 * S[fin] + ehvi_ref.TINY
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(S[fin] > 1e-290, err / S[fin], 0.0)
    print('n=%d M=%d: largest error / S %.3g (allowed 1e-9), largest |error| %.3g, values up to %.3g' % (n, M, ratio.max() if len(ratio) else 0.0,
                                                                                                  err.max() if len(err) else 0.0, np.nanmax(want[fin]) if fin.any() else 0.0))
    for i in np.flatnonzero(~(err <= tol))[:4]:           # (figures first)
        j = np.flatnonzero(fin)[i]
        print('  candidate %d: got %.17g want %.17g S %.6g moments %r' % (j, got[j], want[j], S[j], mom[:, j].tolist()))
    assert np.all(err <= tol)
    assert not np.isfinite(got[~fin]).any() and not np.isfinite(want[~fin]).any()
    if M > 2:
        assert np.isnan(got[0]) and not fin[0] and not fin[1]
    # the order: value descending, index ascending, NaN last
    assert _same((r['top_val'], r['top_idx']), (np.where(np.isnan(got), -np.inf, got)[gp_ref.topk_desc(got, k)], gp_ref.topk_desc(got, k)))
    if M == 257:
        full = lead.ehvi_fold(dmom.data_ptr(), M, P, ref, k=M)
        assert np.array_equal(full['top_idx'], gp_ref.topk_desc(got, M)) and np.isnan(got[full['top_idx'][-1]])
    # a candidate's value depends on its moments alone: permuted candidates give permuted bits, a sub-range the same bits
    if M > 1:
        perm = np.random.RandomState(n + M).permutation(M)
        dperm = _DevBuf(M)
        lead.ehvi_fold(_dev(mom[:, perm]).data_ptr(), M, P, ref, k=0, d_acq=dperm.data_ptr())
        assert _bits(dperm.numpy(), got[perm])
        lo, hi = M // 3, M // 3 + max(1, M // 5)
        dsub = _DevBuf(hi - lo)
        lead.ehvi_fold(_dev(mom[:, lo:hi]).data_ptr(), hi - lo, P, ref, k=0, d_acq=dsub.data_ptr())
        assert _bits(dsub.numpy(), got[lo:hi])
    lead.close()


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_values_and_top_k_against_the_oracle(name):
    from pybo_amd._lib import Engine
    p, (f1, f2) = _case(name)
    Z, k = p['Z'], 10
    P, ref = _data_front(p)
    a, b = ehvi_ref.strips(P, ref)
    v, tol, _ = ehvi_ref.values(ehvi_ref.models(p), a, b, Z)
    r = Engine.ehvi_sweep(f1, f2, P, ref, Z, k=k, want_all=True)
    err = np.abs(r['acq'] - v)
    with np.errstate(divide='ignore', invalid='ignore'):
        print('%s: front of %d, values up to %.4g, worst err %.3g, worst err / tol %.3g' % (name, len(b) - 1, v.max(), err.max(), np.nanmax(err / tol)))
    for i in np.flatnonzero(~(err <= tol))[:4]:
        print('  candidate %d: got %.17g want %.17g tol %.3g' % (i, r['acq'][i], v[i], tol[i]))
    assert np.all(err <= tol) and v.max() > 1e-4
    # the top-k is the lexsort (value descending, index ascending) of the call's own values
    assert _same((r['top_val'], r['top_idx']), _topk_of(r['acq'], k))
    best = int(np.argmax(v))
    top = int(r['top_idx'][0])
    assert best in r['top_idx'] or abs(v[best] - r['top_val'][0]) <= tol[best] + tol[top]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_message_on_the_lead_and_touch_nothing():
    from pybo_amd import _lib
    from pybo_amd._lib import Engine, GpxError
    p = cases.build(300, 3, 'se', 31, m=600)
    f1, f2 = _fit_engines(p)
    twin = _fit_engines(p)[1]                  # f2's twin: the same fit, never part of a refused call
    Z, M = p['Z'], 600
    P, ref = _data_front(p)
    wide = _fit_engines(cases.build(300, 4, 'se', 31, m=8))[0]
    unfitted = Engine(0)
    unfitted.d = 3
    # f2 holds a live sweep cache and a pending announcement; the refused calls must leave both alone
    xnew, ynew = np.full(3, 0.37), 0.2
    for e in (f2, twin):
        e.set_option('sweep_cache', 1)
        e.sweep('ei', 0.1, Z, k=5, want_all=False)
        e.set_option('sweep_cache', 0)
        assert e.append_begin(xnew)
    before = [e.predict(Z[:64]) for e in (f1, f2)]
    swept = f1.sweep('ei', 0.1, Z, k=5, want_all=True)

    def refused(code, a, b, front=P, r=ref, Zc=Z, k=5):
        with pytest.raises(GpxError) as err:
            Engine.ehvi_sweep(a, b, front, r, Zc, k=k, want_all=False)
        assert err.value.code == code and len(str(err.value)) > len('libgpx error %d: ' % code), (code, str(err.value))
        assert 'ehvi_sweep' in str(err.value)              # the message is the lead's

    refused(_lib.GPX_EARG, f1, f1)                                             # one handle twice
    refused(_lib.GPX_EARG, f1, wide)                                           # another input dimension
    refused(_lib.GPX_ESTATE, f1, unfitted)
    refused(_lib.GPX_ESTATE, unfitted, f2)
    for bad in (np.inf, -np.inf, np.nan):
        refused(_lib.GPX_EARG, f1, f2, r=[ref[0], bad])
        Pb = P.copy()
        Pb[7, 0] = bad
        refused(_lib.GPX_EARG, f1, f2, front=Pb)
    refused(_lib.GPX_EARG, f1, f2, front=np.zeros((4097, 2)))                 # raw points: at most 4096
    big, bigref = cases.raw_front(1025, seed=3)
    assert len(big) <= 4096
    refused(_lib.GPX_EARG, f1, f2, front=big, r=bigref)                       # 1025 survive the filter
    refused(_lib.GPX_EARG, f1, f2, Zc=np.empty((0, 3)))                       # M >= 1
    refused(_lib.GPX_EARG, f1, f2, k=4097)
    # raw calls: NULL handles, np < 0, a NULL front with np > 0, a NULL reference point, NULL top-k outputs; the fold's own checks
    lib = _lib.load()
    tv, ti, zz, pp, rr = np.empty(5), np.empty(5, dtype=np.int64), np.ascontiguousarray(Z), np.ascontiguousarray(P), np.ascontiguousarray(ref)
    V = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert lib.gpx_ehvi_sweep(None, f2._h, V(pp), len(P), V(rr), V(zz), M, 5, V(tv), V(ti), None) == _lib.GPX_EARG
    for args in ((f1._h, None, V(pp), len(P), V(rr), V(zz), M, 5, V(tv), V(ti), None), (f1._h, f2._h, V(pp), -1, V(rr), V(zz), M, 5, V(tv), V(ti), None),
                 (f1._h, f2._h, None, 3, V(rr), V(zz), M, 5, V(tv), V(ti), None), (f1._h, f2._h, V(pp), len(P), None, V(zz), M, 5, V(tv), V(ti), None),
                 (f1._h, f2._h, V(pp), len(P), V(rr), None, M, 5, V(tv), V(ti), None), (f1._h, f2._h, V(pp), len(P), V(rr), V(zz), M, 5, None, V(ti), None)):
        assert lib.gpx_ehvi_sweep(*args) == _lib.GPX_EARG and b'ehvi_sweep' in lib.gpx_last_error(f1._h)
    dmom = _dev(cases.synthetic_moments(M, seed=1))
    for kw in (dict(front=big, ref=bigref), dict(front=P, ref=[np.nan, 0.0]), dict(front=P, ref=ref, k=4097)):
        with pytest.raises(GpxError) as err:
            f1.ehvi_fold(dmom.data_ptr(), M, kw['front'], kw['ref'], k=kw.get('k', 5))
        assert err.value.code == _lib.GPX_EARG and 'ehvi_fold' in str(err.value)
    assert lib.gpx_ehvi_fold_dev(f1._h, None, M, V(pp), len(P), V(rr), 5, V(tv), V(ti), None) == _lib.GPX_EARG
    assert lib.gpx_ehvi_fold_dev(f1._h, C.c_void_p(dmom.data_ptr()), 0, V(pp), len(P), V(rr), 5, V(tv), V(ti), None) == _lib.GPX_EARG
    assert lib.gpx_ehvi_fold_dev(None, C.c_void_p(dmom.data_ptr()), M, V(pp), len(P), V(rr), 5, V(tv), V(ti), None) == _lib.GPX_EARG
    # untouched: the fits (a following sweep gives the bits it gave before) ...
    for e, (mu, s2) in zip((f1, f2), before):
        got = e.predict(Z[:64])
        assert np.array_equal(got[0], mu) and np.array_equal(got[1], s2)
    again = f1.sweep('ei', 0.1, Z, k=5, want_all=True)
    assert np.array_equal(again['acq'], swept['acq']) and _same((again['top_val'], again['top_idx']), (swept['top_val'], swept['top_idx']))
    # ... f2's sweep cache and its pending announcement: the append finishes as the twin's does, the cache re-scores to the same bits
    assert f2.sweep_cache_size() == twin.sweep_cache_size() == M
    for e in (f2, twin):
        e.timers(reset=True)
    assert f2.append(xnew, ynew) and twin.append(xnew, ynew)
    ra, rb = f2.sweep_update('ei', 0.1, k=5, want_all=True), twin.sweep_update('ei', 0.1, k=5, want_all=True)
    assert np.array_equal(ra['acq'], rb['acq']) and np.array_equal(ra['top_idx'], rb['top_idx'])
    ta, tb = f2.timers(reset=True), twin.timers(reset=True)
    assert (ta['sweep_trmm_launches'], tb['sweep_trmm_launches']) == (0.0, 0.0)      # no full sweep was needed: the cache survived
    # and a good call works afterwards
    ok = Engine.ehvi_sweep(f1, f2, P, ref, Z, k=5, want_all=True)
    assert _same((ok['top_val'], ok['top_idx']), _topk_of(ok['acq'], 5))


# ---- 6. plug-in ------------------------------------------------------------------------------------------------------------------
def test_acq_topk_on_a_device_grid_and_on_a_host_array():
    from pybo_amd import models, policies
    from pybo_amd._lib import DeviceGrid, Engine
    p = cases.problem('se_d8')
    gps = [models.make_gp(sn2, rho, ell, bias, kernel=kern) for (sn2, rho, ell, bias), kern in zip(p['hypers'], p['kernels'])]
    model = models.MultiObjective(*gps)
    model.add_data(p['X'], p['Y'])
    assert model.ndata == 300 and np.array_equal(model.data[1], p['Y'])
    grid = DeviceGrid('uniform', [[0.0, 1.0]] * p['d'], cases.M, seed=5)
    Zh = np.asarray(grid)
    P, ref = _data_front(p)
    f1, f2 = (m._engine() for m in model.objectives)
    want = Engine.ehvi_sweep(f1, f2, P, ref, Zh, k=0, want_all=True)['acq']
    for k in (1, 10):
        tv, ti = model.acq_topk('ehvi', (P, ref), grid, k)
        assert _same((tv, ti), _topk_of(want, k))
        assert _same(model.acq_topk('ehvi', (P, ref), Zh, k), (tv, ti))             # a host array: the same
    assert model.topk_engine() is f1
    # get_ehvi (gpx_ensemble_predict + the closed form on the host): against the oracle at the stated moment tolerances, as the sweep
    a, b = ehvi_ref.strips(P, ref)
    v, tol, _ = ehvi_ref.values(ehvi_ref.models(p), a, b, Zh[:500])
    assert np.all(np.abs(model.get_ehvi(P, ref, Zh[:500]) - v) <= tol) and np.all(np.abs(want[:500] - v) <= tol)
    f, g = model.get_ehvi(P, ref, Zh[:4], grad=True)
    assert f.shape == (4,) and g.shape == (4, p['d']) and np.all(np.isfinite(g))
    # through the policy: the front is the posterior means at the observations, the index's topk is that call
    index = policies.EHVI(model, None, p['X'])
    kind, (front, r) = index.acq
    assert kind == 'ehvi' and np.array_equal(front, model.predict_mean(p['X'])) and not hasattr(index, 'batch')
    wantp = Engine.ehvi_sweep(f1, f2, front, r, Zh, k=0, want_all=True)['acq']
    assert _same(index.topk(grid, 10), _topk_of(wantp, 10))
    with pytest.raises(ValueError):
        model.acq_topk('ei', 0.0, grid, 1)
    grid.close()


def test_solve_bayesopt_with_device_members_on_a_device_grid(capsys):
    from pybo_amd import models, solve_bayesopt
    from pybo_amd._lib import DeviceGrid
    bounds = [[0.0, 1.0], [0.0, 1.0]]
    model = models.MultiObjective(models.make_gp(1e-4, 1.0, [0.4, 0.4], -0.3), models.make_gp(1e-4, 1.0, [0.4, 0.4], -0.3, kernel='matern5'))

    def objective(x):
        x = np.ravel(x)
        return float(-np.sum((x - 0.2) ** 2)), float(-np.sum((x - 0.8) ** 2))

    X0 = np.random.RandomState(0).rand(36, 2)
    model.add_data(X0, [objective(x) for x in X0])
    grid = DeviceGrid('uniform', bounds, 2000, seed=3)
    xbest, model, info = solve_bayesopt(objective, bounds, model=model, niter=5, policy='ehvi', recommender='pareto',
                                        solver=('lbfgs', {'xgrid': grid, 'nbest': 3}), verbose=True, rng=0)
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('i=')]) == 5
    assert info.y.shape == (len(info.x), 2) and model.ndata == 36 + len(info.x) and len(info.xbest) == 5
    assert isinstance(model.objectives[0], models.GP) and np.all((info.x >= 0.0) & (info.x <= 1.0))
    grid.close()


def test_the_cpu_loop_runs_on_device_members(capsys):
    from pybo_amd import models
    from test_ehvi_cpu import run_loop
    xbest, model, info = run_loop(lambda sn2, rho, ell, bias: models.make_gp(sn2, rho, ell, bias))
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('i=')]) == 12
