"""gpx_constrained_sweep_batch on the device: nb greedy picks of the constrained index -- EI or PI of the
objective folded with every constraint's probability of feasibility, or that probability alone -- on the members' live sweep caches,
target and thresholds frozen and every member conditioned on a pick at its own posterior mean, against the from-scratch greedy of
tests/con_batch_ref.py.  Shapes: the cases of con_cases.py over M = 3001 candidates (N = 300 off the tile grid in three block rows,
N = 1100 in nine, twelve scoring blocks, J = 1 to 3, both starts of the chain) plus M > 262 144 (the scoring kernel's grid-stride loop).

Tolerances: helpers.s2_tol for a member's variance at its pick; for a pick's value con_batch_ref.val_tol, the members' stated tolerances
(test_gpu_batch.acq_tol) propagated to first order through the product as con_ref.values does it."""
import ctypes as C
import os

import numpy as np
import pytest

import con_batch_ref
import con_cases
from helpers import s2_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _member(X, y, kernel, hyp, Z, kind, param):
    """A fitted engine with the hyper-parameters hyp = (sn2, rho, ell, bias) whose sweep cache holds Z."""
    from pybo_amd._lib import Engine
    sn2, rho, ell, bias = hyp
    e = Engine(0)
    e.fit(X, y, kernel, ell, rho, sn2, bias)
    e.set_option('sweep_cache', 1)
    e.sweep(kind, param, Z, k=1, want_all=False)
    e.set_option('sweep_cache', 0)
    return e


def _members(p, kind, Z=None, n=None):
    """(objective engine or None, constraint engines) of a con_cases problem (its first n observations), every cache on Z."""
    Z = p['Z'] if Z is None else Z
    hypers, Y, params = con_batch_ref.members_of(p, kind, n)
    kinds = ([] if kind is None else [kind]) + ['pi'] * p['J']
    engines = [_member(p['X'][:len(Y)], Y[:, m], p['kernel'], hypers[m], Z, kinds[m], params[m]) for m in range(len(hypers))]
    return (None, engines) if kind is None else (engines[0], engines[1:])


def _close(obj, cons):
    for e in ([] if obj is None else [obj]) + list(cons):
        e.close()


def _batch(p, kind, obj, cons, nb):
    from pybo_amd._lib import Engine
    return Engine.constrained_batch(obj, cons, p['thr'], kind or 'ei', con_batch_ref.target_of(p, kind), nb)


def _check_against(p, kind, ref, got):
    hypers, _, params = con_batch_ref.members_of(p, kind)
    rhos = np.array([h[1] for h in hypers])[:, None]
    tol = con_batch_ref.val_tol(kind, params, hypers, ref['mu'], ref['s2'])
    print('margins', ref['margin'])
    print('idx', got['sel_idx'], ref['idx'])
    print('val err / tol', np.abs(got['sel_val'] - ref['val']) / tol)
    print('s2 err / tol', (np.abs(got['sel_s2'] - ref['s2']) / s2_tol(ref['s2'], rhos)).max(axis=1))
    assert con_batch_ref.admitted(ref)                                # the admission condition, on the reference itself
    np.testing.assert_array_equal(got['sel_idx'], ref['idx'])
    assert got['sel_s2'].shape == ref['s2'].shape == (len(hypers), len(ref['idx']))
    assert np.all(np.abs(got['sel_s2'] - ref['s2']) <= s2_tol(ref['s2'], rhos))
    assert np.all(np.abs(got['sel_val'] - ref['val']) <= tol)


# ---- 1. against the from-scratch greedy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(con_batch_ref.CASES))
def test_picks_values_and_member_variances_equal_the_from_scratch_greedy(tag):
    p, kind, nb, ref = con_batch_ref.case(tag)
    obj, cons = _members(p, kind)
    got = _batch(p, kind, obj, cons, nb)
    _close(obj, cons)
    _check_against(p, kind, ref, got)


# ---- 2. bit for bit -------------------------------------------------------------------------------------------------------------------
def test_round_zero_prefixes_repeats_and_untouched_handles():
    from pybo_amd._lib import Engine
    p, kind, nb, ref = con_batch_ref.case('se_j2_ei')
    obj, cons = _members(p, kind)
    thr, Z = p['thr'], p['Z']
    everyone = [(obj, 'ei', p['target'])] + [(c, 'pi', t) for c, t in zip(cons, thr)]
    before = [e.sweep_update(kd, t, k=10, want_moments=True) for e, kd, t in everyone]
    # round 0 is the constrained sweep's winner over the same candidates, value and index, with and without an objective
    for o, acq, param in ((obj, 'ei', p['target']), (obj, 'pi', p['target'] + 0.05), (None, 'ei', None)):
        full = Engine.constrained_sweep(o, cons, thr, acq, param, Z, k=1, want_all=True)
        first = Engine.constrained_batch(o, cons, thr, acq, param, 1)
        assert first['sel_idx'][0] == full['top_idx'][0] and first['sel_val'][0] == full['top_val'][0], (o is not None, acq)
        assert first['sel_val'][0] == full['acq'][full['top_idx'][0]]
        assert first['sel_s2'].shape == (len(cons) + (o is not None), 1)
    long = _batch(p, kind, obj, cons, 8)
    short = _batch(p, kind, obj, cons, 3)
    again = _batch(p, kind, obj, cons, 8)
    np.testing.assert_array_equal(long['sel_idx'], ref['idx'])
    for key in ('sel_val', 'sel_idx'):
        np.testing.assert_array_equal(short[key], long[key][:3])
        np.testing.assert_array_equal(again[key], long[key])
    np.testing.assert_array_equal(short['sel_s2'], long['sel_s2'][:, :3])
    np.testing.assert_array_equal(again['sel_s2'], long['sel_s2'])
    # the prefix property without an objective too
    np.testing.assert_array_equal(_batch(p, None, None, cons, 3)['sel_val'], _batch(p, None, None, cons, 8)['sel_val'][:3])
    # handles and caches are as they were
    for (e, kd, t), upd in zip(everyone, before):
        assert e.sweep_cache_size() == len(Z)
        after = e.sweep_update(kd, t, k=10, want_moments=True)
        for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
            np.testing.assert_array_equal(upd[key], after[key])
    _close(obj, cons)


# ---- 3. factors of exactly 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('acq', ['ei', 'pi'])
def test_thresholds_everyone_clears_give_the_objective_s_own_batch_bit_for_bit(acq):
    """thr = -1e300: every probability of feasibility is exactly 1 and v * 1 = v, so the picks, their values and the objective's variances
    are gpx_sweep_batch's on the objective handle -- while every constraint still runs its own recurrence."""
    from pybo_amd._lib import Engine
    p, kind, nb, ref = con_batch_ref.case('se_j2_ei')
    obj, cons = _members(p, kind)
    target = con_batch_ref.target_of(p, acq)
    want = obj.sweep_batch(acq, target, nb)
    got = Engine.constrained_batch(obj, cons, np.full(p['J'], -1e300), acq, target, nb)
    _close(obj, cons)
    np.testing.assert_array_equal(got['sel_idx'], want['sel_idx'])
    np.testing.assert_array_equal(got['sel_val'], want['sel_val'])
    np.testing.assert_array_equal(got['sel_s2'][0], want['sel_s2'])
    assert np.all(got['sel_s2'][1:] > 0)


# ---- 4. the grid-stride loop ------------------------------------------------------------------------------------------------------------
def test_the_grid_stride_path_beyond_262144_candidates():
    """batch_blocks caps the scoring launch at 1024 blocks of 256: with M > 262 144 every thread takes a second candidate.  262 144
    copies of NON-picked rows in front of the case's candidates can never win a round (the pick is strictly better; a copy ties
    only with its original), so the picks are the case's, shifted, and values and variances are the plain run's bits."""
    p, kind, nb, ref = con_batch_ref.case('se_j1_pi')
    Z = p['Z']
    rest = np.setdiff1d(np.arange(len(Z)), ref['idx'])
    nfill = 262144
    Zbig = np.vstack([Z[rest[np.arange(nfill) % len(rest)]], Z])
    obj, cons = _members(p, kind)
    plain = _batch(p, kind, obj, cons, nb)
    _close(obj, cons)
    obj, cons = _members(p, kind, Zbig)
    big = _batch(p, kind, obj, cons, nb)
    _close(obj, cons)
    np.testing.assert_array_equal(plain['sel_idx'], ref['idx'])
    np.testing.assert_array_equal(big['sel_idx'], nfill + ref['idx'])
    np.testing.assert_array_equal(big['sel_val'], plain['sel_val'])
    np.testing.assert_array_equal(big['sel_s2'], plain['sel_s2'])


# ---- 5. queued appends ------------------------------------------------------------------------------------------------------------------
def test_queued_corrections_are_flushed_first():
    """Every member: fit N = 254, fill the cache, append 3 points WITHOUT re-scoring (their corrections wait in the member's queue,
    its factor crosses the 256-row block boundary), then pick: the reference has 257 observations."""
    p = con_cases.problem('se_j2', m=con_batch_ref.M)
    ref = con_batch_ref.greedy_of(p, 'ei', 8, n=257)
    obj, cons = _members(p, 'ei', n=254)
    cols = np.column_stack([p['y'], p['C']])
    for m, e in enumerate([obj] + cons):
        for i in range(254, 257):
            assert e.append(p['X'][i], cols[i, m])
    got = _batch(p, 'ei', obj, cons, 8)
    _close(obj, cons)
    _check_against(p, 'ei', ref, got)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def _bind(path):
    from pybo_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def test_arguments_and_state_are_refused_alike_by_both_libraries():
    from pybo_amd import _lib
    p = con_cases.build(100, 2, 'se', 5, 2, m=40)
    X = np.ascontiguousarray(p['X'])
    cols = [np.ascontiguousarray(c) for c in np.column_stack([p['y'], p['C']]).T]
    ells = [np.ascontiguousarray(h[2]) for h in p['hypers']]
    rng = np.random.RandomState(0)
    Z, Z30, Zother = np.ascontiguousarray(p['Z']), np.ascontiguousarray(rng.rand(30, 2)), np.ascontiguousarray(rng.rand(40, 2))
    P = _lib._ptr
    codes = {}
    for name in ('libgpx.so', 'libgpx_diag.so'):
        lib = _bind(os.path.join(ROOT, 'pybo_amd', 'csrc', name))
        assert lib.gpx_version() >= 720
        hs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]           # the objective, two constraints
        for h, y, l in zip(hs, cols, ells):
            assert lib.gpx_create(0, None, C.byref(h)) == 0
            assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(l), 1.0, 1e-3, 0.0) == 0
        par, thr = np.array([float(p['target'])]), np.ascontiguousarray(p['thr'])
        sv, si, s2 = np.empty(64), np.empty(64, dtype=np.int64), np.empty(3 * 64)
        tv, ti = np.empty(1), np.empty(1, dtype=np.int64)
        got = []

        def cache(h, Zc):
            assert lib.gpx_set_option(h, b'sweep_cache', 1) == 0
            assert lib.gpx_sweep(h, 0, P(par), 1, P(Zc), len(Zc), 1, P(tv), P(ti), None, None, None) == 0
            assert lib.gpx_set_option(h, b'sweep_cache', 0) == 0

        def call(nb=4, obj=hs[0], cons=None, nc=None, th=thr, acq=0, params=par, nparams=1, v=sv, i=si):
            cons = hs[1:] if cons is None else cons
            arr = (C.c_void_p * max(len(cons), 1))(*[c.value for c in cons])
            rc = lib.gpx_constrained_sweep_batch(obj, arr, len(cons) if nc is None else nc, P(th), acq, P(params), nparams, nb, P(v), P(i), P(s2))
            msg = lib.gpx_last_error(obj if obj is not None else cons[0]) or b''
            assert rc == 0 or len(msg) > 0
            got.append(rc)
            return msg

        cache(hs[0], Z), cache(hs[1], Z)
        msg = call()                                             # constraint 1 has no cache yet: the message names it
        assert got[-1] == _lib.GPX_ESTATE and b'constraint 1' in msg
        msg = call(obj=None)                                     # .. and without an objective it still is constraint 1
        assert got[-1] == _lib.GPX_ESTATE and b'constraint 1' in msg
        cache(hs[2], Z30)
        call()                                                   # caches of different sizes
        cache(hs[2], Zother)
        call()                                                   # equal sizes, different rows
        call(obj=None)
        assert got[2:] == [_lib.GPX_EARG] * 3
        cache(hs[2], Z)
        call()                                                   # the first good call
        assert got[-1] == 0
        good = (sv[:4].copy(), si[:4].copy(), s2[:12].copy())
        mark = len(got)
        call(cons=[hs[1], hs[1]])                                # a handle listed twice
        call(cons=[hs[1], hs[0]])                                # .. the objective among the constraints
        call(cons=[], nc=0)                                      # nc = 0
        call(cons=[hs[1]] * 17, th=np.zeros(17))                 # nc = 17
        call(th=np.array([0.0, np.nan]))                         # a threshold that is not finite
        call(th=np.array([np.inf, 0.0]))
        call(acq=2, params=np.array([2.0]))                      # UCB with an objective
        call(acq=3, params=None, nparams=0)                      # the posterior mean
        call(params=None, nparams=0)                             # no target
        call(nb=0)
        call(nb=65)
        call(nb=41)                                              # nb > M
        call(v=None)                                             # NULL outputs
        call(i=None)
        call(obj=None, nb=0)
        assert got[mark:] == [_lib.GPX_EARG] * 15
        # a refused call leaves nothing behind: the caches are live and the same call returns the same bits
        assert [lib.gpx_sweep_cache_size(h) for h in hs] == [40, 40, 40]
        call()
        assert got[-1] == 0 and np.array_equal(sv[:4], good[0]) and np.array_equal(si[:4], good[1]) and np.array_equal(s2[:12], good[2])
        call(obj=None, acq=2, params=None, nparams=0)            # without an objective acq_id and params are not read
        assert got[-1] == 0 and np.all(sv[:4] <= 1.0) and np.all(sv[:4] >= 0.0)
        call(nb=40)                                              # nb = M: every candidate, each once
        assert got[-1] == 0 and sorted(si[:40].tolist()) == list(range(40))
        assert lib.gpx_fit(hs[2], P(X), 100, 2, P(cols[2]), 0, P(ells[2]), 1.0, 1e-3, 0.0) == 0
        call()                                                   # one constraint refitted: its cache is gone
        assert got[-1] == _lib.GPX_ESTATE
        assert lib.gpx_fit(hs[0], P(X), 100, 2, P(cols[0]), 0, P(ells[0]), 1.0, 1e-3, 0.0) == 0
        msg = call()                                             # the objective's cache: named as such
        assert got[-1] == _lib.GPX_ESTATE and b'objective' in msg
        codes[name] = got
        for h in hs:
            assert lib.gpx_destroy(h) == 0
    assert codes['libgpx.so'] == codes['libgpx_diag.so']


# ---- 7. plug-in -------------------------------------------------------------------------------------------------------------------------
def _device_model(p):
    from pybo_amd import models
    gps = [models.make_gp(sn2, rho, ell, bias, kernel=p['kernel']) for sn2, rho, ell, bias in p['hypers']]
    model = models.Constrained(gps[0], gps[1:], thresholds=p['thr'])
    model.add_data(p['X'], np.column_stack([p['y'], p['C']]))
    return model


@pytest.mark.parametrize('feasible', [True, False])
def test_propose_batch_on_device_members_is_the_one_call_on_their_engines(feasible):
    import pybo_amd
    from pybo_amd import policies
    from pybo_amd._lib import DeviceGrid, Engine
    p = con_cases.problem('se_j1', m=8)
    model = _device_model(p)
    bounds = np.array([[0.0, 1.0]] * p['d'])
    grid = DeviceGrid('uniform', bounds, 3001, seed=5)
    host_grid = np.asarray(grid)
    policy = 'cei' if feasible else ('cei', dict(pmin=1.5))
    index = policies.CEI(model, None, p['X'], **({} if feasible else dict(pmin=1.5)))
    target = index.acq[1]
    assert (target is not None) == feasible and not hasattr(index, 'batch')
    Xq, vals, idx = pybo_amd.propose_batch(model, bounds, p['X'], 8, policy=policy, xgrid=grid)
    members = model._members if feasible else model.constraints
    engines = [m._engine() for m in members]
    assert engines[0].timers()['batch'] > 0 and all(m._state.cache_grid is grid for m in members)
    cold = [e.timers()['sweep_trmm'] for e in engines]
    assert all(t > 0 for t in cold)
    # (the CEI policy scores the feasibility of the observations, a sweep of its own over X on every constraint handle: the second call
    #  is handed the index built above, so that between the two readings of slot 5 nothing but propose_batch's own work can sweep)
    Xq2, vals2, idx2 = pybo_amd.propose_batch(model, bounds, p['X'], 8, policy=lambda m, b, x: index, xgrid=grid)
    assert [e.timers()['sweep_trmm'] for e in engines] == cold      # the second call only re-used the caches: no cold sweep
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(vals, vals2)
    np.testing.assert_array_equal(Xq, host_grid[idx])
    direct = Engine.constrained_batch(engines[0] if feasible else None, engines[1:] if feasible else engines, model.thresholds, 'ei', target, 8)
    np.testing.assert_array_equal(idx, direct['sel_idx'])
    np.testing.assert_array_equal(vals, direct['sel_val'])
    assert len(set(idx.tolist())) == 8
    # a host array takes the device path too (one copy for all members) and picks the same rows
    Xq3, vals3, idx3 = pybo_amd.propose_batch(model, bounds, p['X'], 8, policy=policy, xgrid=host_grid)
    np.testing.assert_array_equal(idx3, idx)
    np.testing.assert_array_equal(vals3, vals)
    with pytest.raises(ValueError, match='constrained'):
        pybo_amd.propose_batch(model, bounds, p['X'], 8, policy=policy, xgrid=grid, fantasies=4)
    grid.close()


def test_the_loop_in_batches_on_a_constrained_device_model():
    import pybo_amd
    from pybo_amd import models
    from pybo_amd._lib import DeviceGrid
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    model = models.Constrained(models.make_gp(1e-4, 1.0, [0.3, 0.3], -0.2), [models.make_gp(1e-4, 1.0, [0.4, 0.4], 0.0)], thresholds=[0.0])
    grid = DeviceGrid('uniform', bounds, 2000, seed=2)

    def objective(x):
        x = np.ravel(x)
        return float(-np.sum((x - 0.3) ** 2)), float(x[0] - 0.5)

    xbest, model, info = pybo_amd.solve_bayesopt(objective, bounds, model=model, niter=12, policy='cei', recommender='feasible', nbatch=4,
                                                 batch_grid=grid, rng=0)
    assert model.ndata == 1 + 12 and len(info.x) == 13 and info.y.shape == (13, 2) and len(info.xbest) == 12
    assert np.array_equal(info.y[:, 1], info.x[:, 0] - 0.5)
    host_grid = np.asarray(grid)
    assert all(any(np.array_equal(x, z) for z in host_grid) for x in info.x[1:])      # every evaluation after the seed is a grid point
    assert model.constraints[0]._engine().timers()['batch'] + model.objective._engine().timers()['batch'] > 0      # the device path
    grid.close()
