"""Constrained sweeps on the device: gpx_constrained_sweep[_dev] returns EI / PI of the objective folded with
every constraint's probability of feasibility, BIT FOR BIT the con_fold chain over the members' own gpx_sweep values; its
selection-only form returns bit for bit what the loop over every candidate returns, and the objective's EI bound holds on every
candidate it leaves out.  The shapes are those of con_cases.py (the oracle's survivor counts for them: test_con_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import gp_ref
import con_cases as cases
import con_ref
from test_gpu_prune import _dev, _DevBuf
from test_gpu_ens_prune import _dev_cand, _check_bound, _same, _topk_of

pytestmark = pytest.mark.gpu


def _fit_engines(p, n=None):
    from pybo_amd._lib import Engine
    n = len(p['X']) if n is None else n
    engines = []
    for i, (sn2, rho, ell, bias) in enumerate(p['hypers']):
        e = Engine(0)
        e.fit(p['X'][:n], (p['y'] if i == 0 else p['C'][:, i - 1])[:n], p['kernel'], ell, rho, sn2, bias)
        engines.append(e)
    return engines


_CASE = {}


def _case(name):
    """The case's problem, fitted engines [objective, constraints ..] (once per session) and every candidate's exact cEI."""
    if name not in _CASE:
        p = cases.problem(name)
        engines = _fit_engines(p)
        vals = _csweep(p, engines, p['Z'], 0, 0, want_all=True)[2]
        _CASE[name] = (p, engines, vals)
    p, engines, vals = _CASE[name]
    for e in engines:
        e.set_option('prune', -1)
        e.set_option('sweep_cache', -1)
    return p, engines, vals


def _csweep(p, engines, Z, k, prune, want_all=False, dev=True, thr=None, acq='ei', target=None):
    """(top_val, top_idx, acq_all or None, report) of one constrained sweep with the objective's option prune set."""
    from pybo_amd._lib import Engine
    engines[0].set_option('prune', prune)
    thr = p['thr'] if thr is None else thr
    target = p['target'] if target is None else target
    if want_all:
        r = Engine.constrained_sweep(engines[0], engines[1:], thr, acq, target, Z, k=k, want_all=True)
    else:
        r = Engine.constrained_sweep(engines[0], engines[1:], thr, acq, target, _dev_cand(Z) if dev else Z, k=k, want_all=False)
    return r['top_val'], r['top_idx'], r['acq'], engines[0].constrained_prune_report()


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('acq', ['ei', 'pi'])
@pytest.mark.parametrize('J', [1, 2, 3])
def test_values_are_the_fold_of_the_members_own_sweeps(J, acq):
    from pybo_amd._lib import Engine
    p = cases.build(300, 3, 'se', 21 + J, J, m=1000)
    engines = _fit_engines(p)
    obj, cons = engines[0], engines[1:]
    Z, thr, target, M, k = p['Z'], p['thr'], p['target'], 1000, 10
    a = obj.sweep(acq, target, Z, k=0)['acq']
    P = [c.sweep('pi', t, Z, k=0)['acq'] for c, t in zip(cons, thr)]
    want_v, want_w = con_ref.chain(a, P), con_ref.pof_chain(P)
    r = Engine.constrained_sweep(obj, cons, thr, acq, target, Z, k=k, want_all=True, want_pof=True)
    assert np.array_equal(r['acq'], want_v) and np.array_equal(r['pof'], want_w)
    assert _same((r['top_val'], r['top_idx']), _topk_of(want_v, k))
    assert obj.constrained_prune_report()['path'] == 'plain'           # a per-candidate call never prunes
    # against the oracle, at the stated moment tolerances propagated through the product (con_ref.py)
    ro, rc = con_ref.models(p)
    v, w, tv, tw = con_ref.values(ro, rc, thr, acq, target, Z)
    ev, ew = np.abs(r['acq'] - v), np.abs(r['pof'] - w)
    with np.errstate(divide='ignore', invalid='ignore'):
        print('J=%d %s: worst err / tol %.3g (value), %.3g (feasibility)' % (J, acq, np.nanmax(ev / tv), np.nanmax(ew / tw)))
    for i in np.flatnonzero((ev > tv) | (ew > tw))[:4]:          # (figures first)
        print('  candidate %d: value %.17g want %.17g tol %.3g | pof %.17g want %.17g tol %.3g' % (i, r['acq'][i], v[i], tv[i], r['pof'][i], w[i], tw[i]))
        for j, (c, rcj) in enumerate(zip(cons, rc)):
            mo = rcj.predict(Z[i:i + 1])
            print('    constraint %d: P %.17g, oracle mu %.17g s2 %.17g z %.6g' % (j, P[j][i], mo[0][0], mo[1][0], (mo[0][0] - thr[j]) / np.sqrt(mo[1][0])))
    assert np.all(ev <= tv) and np.all(ew <= tw)
    assert w.min() < 0.1 and w.max() > 0.9 and v.max() > 1e-3          # the factors do something here, and not everything is 0
    # no objective: the value IS the probability of feasibility; acq_id and params are not read
    n = Engine.constrained_sweep(None, cons, thr, 'ucb', None, Z, k=k, want_all=True, want_pof=True)
    assert np.array_equal(n['acq'], want_w) and np.array_equal(n['pof'], want_w)
    assert _same((n['top_val'], n['top_idx']), _topk_of(want_w, k))
    assert cons[0].constrained_prune_report()['path'] == 'plain'
    # the device form: the same bits in the caller's vectors
    for o in (obj, None):
        dacq, dpof = _DevBuf(M), _DevBuf(M)
        d = Engine.constrained_sweep(o, cons, thr, acq, target, _dev_cand(Z), k=k, d_acq=dacq.data_ptr(), d_pof=dpof.data_ptr())
        ref = r if o is not None else n
        assert np.array_equal(dacq.numpy(), ref['acq']) and np.array_equal(dpof.numpy(), ref['pof'])
        assert _same((d['top_val'], d['top_idx']), (ref['top_val'], ref['top_idx']))
        # and with one or no vector asked for
        only = Engine.constrained_sweep(o, cons, thr, acq, target, _dev_cand(Z), k=k, d_pof=dpof.data_ptr())
        assert _same((only['top_val'], only['top_idx']), (ref['top_val'], ref['top_idx'])) and np.array_equal(dpof.numpy(), ref['pof'])
        none = Engine.constrained_sweep(o, cons, thr, acq, target, _dev_cand(Z), k=k)
        assert _same((none['top_val'], none['top_idx']), (ref['top_val'], ref['top_idx']))
    # the order of the constraints is the caller's: the product in another order is another rounding
    if J > 1:
        back = Engine.constrained_sweep(obj, cons[::-1], thr[::-1], acq, target, Z, k=0, want_all=True)['acq']
        assert np.array_equal(back, con_ref.chain(a, P[::-1]))


# ---- 2. order ----------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_index_and_nan_ranks_last():
    from pybo_amd._lib import Engine
    p = cases.build(300, 3, 'se', 23, 2, m=1000)
    engines = _fit_engines(p)
    Z = p['Z'].copy()
    base = Engine.constrained_sweep(engines[0], engines[1:], p['thr'], 'ei', p['target'], Z, k=3, want_all=True)
    b0, b1 = int(base['top_idx'][0]), int(base['top_idx'][1])
    Z[[900, 5, 412]] = Z[b0]
    Z[[77, 650]] = Z[b1]
    Z[300, 1] = np.nan
    M = len(Z)
    r = Engine.constrained_sweep(engines[0], engines[1:], p['thr'], 'ei', p['target'], Z, k=M, want_all=True)
    v = r['acq']
    assert np.isnan(v[300]) and np.isnan(v).sum() == 1
    assert np.array_equal(r['top_idx'], gp_ref.topk_desc(v, M)) and np.array_equal(r['top_val'], np.where(np.isnan(v), -np.inf, v)[r['top_idx']])
    assert [int(i) for i in r['top_idx'][:4]] == sorted([5, 412, 900, b0]) and r['top_idx'][-1] == 300
    assert [int(i) for i in r['top_idx'][4:7]] == sorted([77, 650, b1])
    d = Engine.constrained_sweep(engines[0], engines[1:], p['thr'], 'ei', p['target'], _dev_cand(Z), k=M)
    assert _same((d['top_val'], d['top_idx']), (r['top_val'], r['top_idx']))


# ---- 3. pruned against plain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', cases.KS)
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_pruned_and_plain_paths_agree_and_the_bound_holds_on_every_candidate(name, k):
    p, engines, vals = _case(name)
    want = _topk_of(vals, k)
    for dev in (True, False):
        plain = _csweep(p, engines, p['Z'], k, 0, dev=dev)
        pruned = _csweep(p, engines, p['Z'], k, 1, dev=dev)
        assert _same(plain, pruned) and _same(pruned, want), (name, k, dev)
        assert plain[3]['path'] == 'plain'
        rep = pruned[3]
        print('%s k=%d %s: survivors %d, tau %.4g, delta %.3g' % (name, k, 'dev' if dev else 'host', rep['nsurv'], rep['tau'], rep['delta']))
        assert rep['path'] == 'pruned' and rep['done'] == 0 and np.isnan(rep['gate'])
        assert rep['G'] == cases.G and rep['cap'] == cases.cap_of(len(vals)) and rep['nsurv'] <= rep['cap'] and rep['delta'] > 0
    # ub[n] >= value[n] for EVERY candidate not evaluated as a seed; what is left out cannot be among the k best
    _check_bound(rep, vals)
    seeds = np.flatnonzero(np.isneginf(rep['ub']))
    assert len(seeds) == cases.G and rep['tau'] == np.sort(vals[seeds])[::-1][k - 1]
    # the work went away: the constraints swept seeds and survivors only, the objective nothing else either
    for e in engines:
        e.timers(reset=True)
    _csweep(p, engines, p['Z'], k, 1)
    N = float(p['N'])
    for e in engines:
        assert e.timers(reset=True)['sweep_trmm_flop'] == pytest.approx(N * N * (cases.G + rep['nsurv']), rel=1e-12)


def test_a_pruned_sweep_may_be_the_first_use_of_the_objective_s_fit():
    """gpx_fit stops at the factorisation; the inverse and `a` follow on first use.  With prune = 1 the bound pass is the first reader of
    the objective's: freshly created and fitted handles, no call between the fit and the selection-only sweep -- and the same on handles
    that held ANOTHER model before (a stale inverse would bound with that model's weights)."""
    name = 'se_j2'
    p, _, vals = _case(name)
    other = cases.build(p['N'], p['d'], p['kernel'], 77, p['J'], m=1)
    for k in (1, 10):
        want = _topk_of(vals, k)
        for refit in (False, True):
            engines = _fit_engines(other) if refit else None
            if refit:
                _csweep(other, engines, p['Z'], k, 0)               # the other model's inverse and `a` are in the buffers
                for i, (e, (sn2, rho, ell, bias)) in enumerate(zip(engines, p['hypers'])):
                    e.fit(p['X'], p['y'] if i == 0 else p['C'][:, i - 1], p['kernel'], ell, rho, sn2, bias)
            else:
                engines = _fit_engines(p)
            first = _csweep(p, engines, p['Z'], k, 1)
            assert first[3]['path'] == 'pruned' and _same(first, want), (k, refit)
            _check_bound(first[3], vals)
            assert _same(_csweep(p, engines, p['Z'], k, 0), first)
            for e in engines:
                e.close()


# ---- 4. fallback, 5. the size rule ---------------------------------------------------------------------------------------------
def test_thresholds_nobody_reaches_fall_back_to_the_plain_loop():
    """Thresholds at max(c_j) + 10: the probability of feasibility is about 0 everywhere, the objective's bound says nothing about the
    product, more than cap candidates survive and the plain loop runs (path 3), with the results of prune = 0.  Measured on the device:
    tau = 6.2e-78, 8905 survivors of 13001 against cap 4096.  (Ten units above the data is 8 to 12 posterior standard deviations here:
    the values are around 1e-65, not below 1e-280 -- the fallback is the survivor count's, not the tau < 1e-280 rule's.  That rule is
    exercised by the second half: thresholds at max(c_j) + 1000 underflow every probability to 0, tau = 0.)"""
    name, k = 'se_j2', 10
    p, engines, _ = _case(name)
    thr = p['C'].max(axis=0) + 10.0
    vals = _csweep(p, engines, p['Z'], 0, 0, want_all=True, thr=thr)[2]
    plain = _csweep(p, engines, p['Z'], k, 0, thr=thr)
    pruned = _csweep(p, engines, p['Z'], k, 1, thr=thr)
    assert _same(plain, pruned) and _same(pruned, _topk_of(vals, k))
    rep = pruned[3]
    print('thresholds + 10: tau %.4g, survivors %d, cap %d' % (rep['tau'], rep['nsurv'], rep['cap']))
    assert rep['path'] == 'fell back' and rep['nsurv'] > rep['cap']
    fin = np.isfinite(rep['ub'])
    assert np.all(rep['ub'][fin] >= vals[fin]) and np.isneginf(rep['ub']).sum() == cases.G
    # thresholds so far out that every probability underflows: every value is 0, tau = 0 < 1e-280 prunes nothing
    far = p['C'].max(axis=0) + 1000.0
    zero = _csweep(p, engines, p['Z'], 0, 0, want_all=True, thr=far)[2]
    assert np.all(zero == 0.0)
    plain, pruned = _csweep(p, engines, p['Z'], k, 0, thr=far), _csweep(p, engines, p['Z'], k, 1, thr=far)
    assert _same(plain, pruned) and np.array_equal(pruned[1], np.arange(k))
    assert pruned[3]['path'] == 'fell back' and pruned[3]['tau'] == 0.0 and pruned[3]['nsurv'] > pruned[3]['cap']


def test_the_size_rule_declines_small_sweeps():
    name, k = 'se_j2_n9', 10
    p, engines, vals = _case(name)
    auto = _csweep(p, engines, p['Z'], k, -1)
    assert auto[3]['path'] == 'plain' and _same(auto, _topk_of(vals, k))
    # nothing but EI of the objective for the top-k alone is pruned; a sweep cache on any handle forbids it
    assert _csweep(p, engines, p['Z'], k, 1, acq='pi')[3]['path'] == 'plain'
    assert _csweep(p, engines, p['Z'][:3 * cases.G - 1], k, 1)[3]['path'] == 'plain'
    assert _csweep(p, engines, p['Z'][:3 * cases.G], k, 1)[3]['path'] == 'pruned'
    engines[2].set_option('sweep_cache', 1)
    cached = _csweep(p, engines, p['Z'], k, 1)
    assert cached[3]['path'] == 'plain' and _same(cached, _topk_of(vals, k)) and engines[2].sweep_cache_size() == len(p['Z'])
    engines[2].set_option('sweep_cache', -1)
    # the report's vectors lie in the lead's pruning workspace: a later selection-only sweep of the lead alone that lays it out ends the record
    from pybo_amd._lib import GpxError, GPX_ESTATE
    assert _csweep(p, engines, p['Z'], k, 1)[3]['path'] == 'pruned'
    dZ = _dev(p['Z'])
    engines[0].sweep_dev('ei', p['target'], dZ.data_ptr(), len(p['Z']), k)
    assert engines[0].prune_report(vectors=False)['path'] in ('pruned', 'fell back')
    with pytest.raises(GpxError) as gone:
        engines[0].constrained_prune_report()
    assert gone.value.code == GPX_ESTATE


# ---- 6. handle history -----------------------------------------------------------------------------------------------------------
def test_appended_handles_sweep_like_freshly_fitted_ones():
    """N = 1151 + 2 (matern5) crosses a block row: the last two observations appended to the objective and to every constraint.  Each
    handle's moments are stated to mu_tol / s2_tol whatever its history, so both sweeps lie within con_ref's propagated tolerance of
    the oracle, and within twice that of each other."""
    p = cases.build(1153, 8, 'matern5', 11, 2)
    k = 10
    grown = _fit_engines(p, 1151)
    for i, e in enumerate(grown):
        for n in (1151, 1152):
            assert e.append(p['X'][n], float((p['y'] if i == 0 else p['C'][:, i - 1])[n]))
    fresh = _fit_engines(p)
    vg = _csweep(p, grown, p['Z'], 0, 0, want_all=True)[2]
    vf = _csweep(p, fresh, p['Z'], 0, 0, want_all=True)[2]
    ro, rc = con_ref.models(p)
    v, _, tv, _ = con_ref.values(ro, rc, p['thr'], 'ei', p['target'], p['Z'])          # every candidate
    print('appended: worst err / tol %.3g; fresh %.3g; appended against fresh %.3g of 2 tol'
          % ((np.abs(vg - v) / tv).max(), (np.abs(vf - v) / tv).max(), (np.abs(vg - vf) / (2 * tv)).max()))
    assert np.all(np.abs(vg - v) <= tv) and np.all(np.abs(vf - v) <= tv) and np.all(np.abs(vg - vf) <= 2 * tv)
    plain = _csweep(p, grown, p['Z'], k, 0)
    pruned = _csweep(p, grown, p['Z'], k, 1)
    print('appended, prune = 1: %s, survivors %d' % (pruned[3]['path'], pruned[3]['nsurv']))
    assert _same(plain, pruned) and _same(pruned, _topk_of(vg, k)) and pruned[3]['path'] in ('pruned', 'fell back')
    if pruned[3]['path'] == 'pruned':
        _check_bound(pruned[3], vg)


# ---- 7. contract -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_message_clear_the_report_and_touch_nothing():
    from pybo_amd import _lib
    from pybo_amd._lib import Engine, GpxError
    p = cases.build(300, 3, 'se', 31, 2, m=600)
    obj, c0, c1 = _fit_engines(p)
    twin = _fit_engines(p)[1]                  # c0's twin: the same fit, never part of a refused call
    Z, thr, t = p['Z'], p['thr'], p['target']
    other_d = cases.build(300, 4, 'se', 31, 1, m=8)
    wide = _fit_engines(other_d)[0]
    unfitted = Engine(0)
    unfitted.d = 3
    # c0 holds a live sweep cache and a pending announcement; the refused calls must leave both alone
    xnew, ynew = np.full(3, 0.37), 0.2
    for e in (c0, twin):
        e.set_option('sweep_cache', 1)
        e.sweep('pi', thr[0], Z, k=5, want_all=False)
        e.set_option('sweep_cache', 0)
        assert e.append_begin(xnew)
    before = [e.predict(Z[:64]) for e in (obj, c0, c1)]
    ok = Engine.constrained_sweep(obj, [c1], thr[1:], 'ei', t, Z, k=5, want_all=False)
    assert obj.constrained_prune_report(vectors=False)['path'] == 'plain'

    def refused(code, o, cons, th, acq='ei', param=t, Zc=Z, k=5):
        lead = o if o is not None else cons[0]
        with pytest.raises(GpxError) as err:
            Engine.constrained_sweep(o, cons, th, acq, param, Zc, k=k, want_all=False)
        assert err.value.code == code and len(str(err.value)) > len('libgpx error %d: ' % code), (code, str(err.value))
        with pytest.raises(GpxError) as rep:             # a refused call clears the lead's report
            lead.constrained_prune_report()
        assert rep.value.code == _lib.GPX_ESTATE

    refused(_lib.GPX_EARG, obj, [c0] * 17, np.zeros(17))                       # 1 <= nc <= 16
    refused(_lib.GPX_EARG, obj, [c0, c0], thr)                                 # a repeated handle
    refused(_lib.GPX_EARG, obj, [c0, obj], thr)
    refused(_lib.GPX_EARG, None, [c0, c1, c0], np.zeros(3))
    refused(_lib.GPX_ESTATE, obj, [c0, unfitted], thr)                         # an unfitted handle
    refused(_lib.GPX_ESTATE, unfitted, [c0], thr[:1])
    refused(_lib.GPX_EARG, obj, [c0, wide], thr)                               # another input dimension
    for acq, param in (('ucb', 2.0), ('mean', None), ('mes', [t, t + 0.1]), ('kg', Z[:2])):
        refused(_lib.GPX_EARG, obj, [c0, c1], thr, acq=acq, param=param)       # only EI and PI are non-negative
    refused(_lib.GPX_EARG, obj, [c0, c1], np.array([0.0, np.inf]))             # thresholds: finite
    refused(_lib.GPX_EARG, obj, [c0, c1], np.array([np.nan, 0.0]))
    refused(_lib.GPX_EARG, obj, [c0, c1], thr, k=4097)
    refused(_lib.GPX_EARG, None, [c0, c1], thr, Zc=np.empty((0, 3)))           # M >= 1
    # raw calls: no constraint list, NULL thresholds, a NULL constraint
    lib = _lib.load()
    tv, ti, zz = np.empty(5), np.empty(5, dtype=np.int64), np.ascontiguousarray(Z)
    one = (C.c_void_p * 2)(c0._h, None)
    th = np.ascontiguousarray(thr)
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    par = np.array([t])
    assert lib.gpx_constrained_sweep(obj._h, None, 0, P(th), 0, P(par), 1, P(zz), len(Z), 5, P(tv), P(ti), None, None) == _lib.GPX_EARG
    assert lib.gpx_last_error(obj._h)
    assert lib.gpx_constrained_sweep(obj._h, one, 2, P(th), 0, P(par), 1, P(zz), len(Z), 5, P(tv), P(ti), None, None) == _lib.GPX_EARG
    assert lib.gpx_constrained_sweep(obj._h, one, 1, None, 0, P(par), 1, P(zz), len(Z), 5, P(tv), P(ti), None, None) == _lib.GPX_EARG
    assert lib.gpx_constrained_sweep(obj._h, one, 1, P(th), 0, None, 0, P(zz), len(Z), 5, P(tv), P(ti), None, None) == _lib.GPX_EARG
    assert lib.gpx_constrained_sweep(None, None, 0, P(th), 0, P(par), 1, P(zz), len(Z), 5, P(tv), P(ti), None, None) == _lib.GPX_EARG
    # untouched: the fits ...
    for e, (mu, s2) in zip((obj, c0, c1), before):
        got = e.predict(Z[:64])
        assert np.array_equal(got[0], mu) and np.array_equal(got[1], s2)
    # ... c0's sweep cache and its pending announcement: the append finishes as the twin's does, the cache re-scores to the same bits
    assert c0.sweep_cache_size() == twin.sweep_cache_size() == len(Z)
    for e in (c0, twin):
        e.timers(reset=True)
    assert c0.append(xnew, ynew) and twin.append(xnew, ynew)
    ra, rb = c0.sweep_update('pi', thr[0], k=5, want_all=True), twin.sweep_update('pi', thr[0], k=5, want_all=True)
    assert np.array_equal(ra['acq'], rb['acq']) and np.array_equal(ra['top_idx'], rb['top_idx'])
    ta, tb = c0.timers(reset=True), twin.timers(reset=True)
    assert (ta['sweep_trmm_launches'], tb['sweep_trmm_launches']) == (0.0, 0.0)      # no full sweep was needed: the cache survived
    # and a good call still works afterwards, to the same bits as before
    again = Engine.constrained_sweep(obj, [c1], thr[1:], 'ei', t, Z, k=5, want_all=False)
    assert _same((ok['top_val'], ok['top_idx']), (again['top_val'], again['top_idx']))


# ---- 8. plug-in ------------------------------------------------------------------------------------------------------------------
def _device_model(p):
    from pybo_amd import models
    gps = [models.make_gp(sn2, rho, ell, bias, kernel=p['kernel']) for sn2, rho, ell, bias in p['hypers']]
    model = models.Constrained(gps[0], gps[1:], thresholds=p['thr'])
    model.add_data(p['X'], np.column_stack([p['y'], p['C']]))
    return model


def test_acq_topk_on_a_device_grid_equals_the_composition_of_the_members_values():
    from pybo_amd import policies
    from pybo_amd._lib import DeviceGrid
    p = cases.problem('se_j2')
    model = _device_model(p)
    grid = DeviceGrid('uniform', [[0.0, 1.0]] * p['d'], cases.M, seed=5)
    Zh = np.asarray(grid)
    for target in (p['target'], None):
        a = 1.0 if target is None else model.objective.acq_values('ei', target, Zh)
        want = con_ref.chain(a, [c.acq_values('pi', t, Zh) for c, t in zip(model.constraints, model.thresholds)])
        for k in (1, 10):
            tv, ti = model.acq_topk('cei', target, grid, k)
            assert _same((tv, ti), _topk_of(want, k))
            assert _same(model.acq_topk('cei', target, Zh, k), (tv, ti))             # a host array: the same
        lead = model.topk_engine()
        assert lead is (model.objective if target is not None else model.constraints[0])._engine()
        assert np.array_equal(model.get_constrained(target, Zh[:500]), want[:500])
    # through the policy: the index's topk is that call, its target the best probably-feasible observation
    index = policies.CEI(model, None, p['X'])
    ok = model.feasibility(p['X']) >= 0.5
    assert index.acq == ('cei', model.predict_mean(p['X'])[ok].max()) and not hasattr(index, 'batch')
    a = model.objective.acq_values('ei', index.acq[1], Zh)
    want = con_ref.chain(a, [c.acq_values('pi', t, Zh) for c, t in zip(model.constraints, model.thresholds)])
    assert _same(index.topk(grid, 10), _topk_of(want, 10))
    grid.close()


def test_get_constrained_with_gradients():
    """Values: con_ref's propagated tolerance.  Gradients: con_ref.grad_tol, the stated tolerances of the members' moments and of their
    gradients propagated to first order through the closed forms and the product rule; and central differences of the oracle's value."""
    p = cases.build(300, 3, 'se', 41, 2, m=400)
    model = _device_model(p)
    ro, rc = con_ref.models(p)
    for target in (p['target'], None):
        members, ts = ([ro] if target is not None else []) + rc, ([target] if target is not None else []) + list(p['thr'])
        # the 12 candidates where the index moves most: at most of the others it is flat at 0 or 1
        Z = p['Z'][gp_ref.topk_desc(np.abs(con_ref.value_grad(ro, rc, p['thr'], target, p['Z'])[1]).max(axis=1), 12)]
        f, g = model.get_constrained(target, Z, grad=True)
        fr, gr = con_ref.value_grad(ro, rc, p['thr'], target, Z)
        fm, gm = con_ref.value_grad_from_moments([m.predict(Z, grad=True) for m in members], ts, target is not None)
        np.testing.assert_allclose(fm, fr, rtol=1e-12, atol=0)
        np.testing.assert_allclose(gm, gr, rtol=1e-10, atol=1e-14)
        v, w, tv, tw = con_ref.values(ro, rc, p['thr'], 'ei' if target is not None else None, target, Z)
        assert np.all(np.abs(f - v) <= tv) and np.all(np.abs(f - model.get_constrained(target, Z)) <= 2 * tv)
        tol = con_ref.grad_tol(members, ts, target is not None, Z)
        with np.errstate(divide='ignore', invalid='ignore'):
            print('target %s: |g| up to %.3g, worst gradient err %.3g, err / tol %.3g' % (target, np.abs(gr).max(), np.abs(g - gr).max(), np.nanmax(np.abs(g - gr) / tol)))
        assert np.all(np.abs(g - gr) <= tol) and np.abs(gr).max() > 1e-2 and np.all(tol <= 1e-3 * np.abs(gr).max())
        h = 1e-6
        for j in range(Z.shape[1]):
            e = np.zeros(Z.shape[1])
            e[j] = h
            num = (con_ref.value_grad(ro, rc, p['thr'], target, Z + e)[0] - con_ref.value_grad(ro, rc, p['thr'], target, Z - e)[0]) / (2 * h)
            assert np.all(np.abs(g[:, j] - num) <= tol[:, j] + 1e-5 * np.abs(gr).max())
    fw, gw = model.feasibility(Z, grad=True)
    assert np.array_equal(fw, f) and np.array_equal(gw, g)


def test_solve_bayesopt_with_device_members(capsys):
    from pybo_amd import models
    from test_con_cpu import run_loop
    xbest, model, info = run_loop(lambda sn2, rho, ell, bias: models.make_gp(sn2, rho, ell, bias))
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('i=')]) == 12
    assert isinstance(model.objective, models.GP) and model.ndata == len(info.x)
