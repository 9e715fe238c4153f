"""gpx_ehvi_sweep_batch on the device: nb greedy picks of the expected hypervolume improvement on the two members'
live sweep caches, members and reference point frozen, each member conditioned on a pick at its own posterior mean and the pick's believed
outcome taken into the front ON THE DEVICE before the next round -- against the from-scratch greedy of tests/ehvi_batch_ref.py.  Shapes:
ehvi_cases over M = 3001 candidates (N = 300 off the tile grid in three block rows, twelve scoring blocks), fronts of 0 to 1021 points that
lose runs of up to 900 points, grow, or stay (the cap n + nb - 1 = 1024 exactly), plus M > 262 144 (the scoring kernel's grid-stride loop).

Tolerances: helpers.mu_tol / s2_tol for a member's moments at its pick; for a pick's value ehvi_batch_ref.val_tol -- ehvi_ref.values' own
plus the first-order effect of the believed coordinates inserted so far, each moved by its mu_tol.  The picks, the sizes of the front and
everything device against device are compared exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import ehvi_batch_ref
import ehvi_cases
from helpers import mu_tol, s2_tol
from test_gpu_prune import _dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members(p, ref, Z=None, n=None):
    """The two fitted engines of an ehvi_cases problem (its first n observations), each one's sweep cache on Z."""
    from pybo_amd._lib import Engine
    Z = p['Z'] if Z is None else Z
    n = len(p['X']) if n is None else n
    engines = []
    for j, (sn2, rho, ell, bias) in enumerate(p['hypers']):
        e = Engine(0)
        e.fit(p['X'][:n], p['Y'][:n, j], p['kernels'][j], ell, rho, sn2, bias)
        e.set_option('sweep_cache', 1)
        e.sweep('ei', float(ref[j]), Z, k=1, want_all=False)
        e.set_option('sweep_cache', 0)
        engines.append(e)
    return engines


def _close(engines):
    for e in engines:
        e.close()


def _check_against(p, r, got):
    rhos = [h[1] for h in p['hypers']]
    tol = ehvi_batch_ref.val_tol(p, r)
    want_y, want_s2 = r['mom'][:, [0, 2]], r['mom'][:, [1, 3]].T
    ytol = np.column_stack([mu_tol(want_y[:, c], rhos[c]) for c in range(2)])
    stol = np.array([s2_tol(want_s2[c], rhos[c]) for c in range(2)])
    print('margins', r['margin'])
    print('idx', got['sel_idx'], r['idx'])
    print('nfront', got['sel_nfront'], r['n'])
    print('val err / tol', np.abs(got['sel_val'] - r['val']) / tol)
    print('y err / tol', (np.abs(got['sel_y'] - want_y) / ytol).max(axis=0), 's2 err / tol', (np.abs(got['sel_s2'] - want_s2) / stol).max(axis=1))
    assert ehvi_batch_ref.admitted(p, r)                               # the admission condition, on the reference itself
    np.testing.assert_array_equal(got['sel_idx'], r['idx'])
    np.testing.assert_array_equal(got['sel_nfront'], r['n'])
    assert got['sel_y'].shape == want_y.shape and got['sel_s2'].shape == want_s2.shape
    assert np.all(np.abs(got['sel_y'] - want_y) <= ytol)
    assert np.all(np.abs(got['sel_s2'] - want_s2) <= stol)
    assert np.all(np.abs(got['sel_val'] - r['val']) <= tol)


# ---- 1. against the from-scratch greedy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(t for t in ehvi_batch_ref.CASES if not t.endswith('n257')))
def test_picks_fronts_values_and_member_moments_equal_the_from_scratch_greedy(tag):
    from pybo_amd._lib import Engine
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case(tag)
    f1, f2 = _members(p, ref)
    got = Engine.ehvi_batch(f1, f2, P, ref, nb)
    _close([f1, f2])
    _check_against(p, r, got)


# ---- 2. bit for bit, device against device ------------------------------------------------------------------------------------------
def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('tag', ['m5_d6_stair256', 'se_d8_empty', 'se_d8_means'])
def test_round_zero_believed_outcomes_values_prefixes_repeats_and_untouched_handles(tag):
    from pybo_amd._lib import Engine
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case(tag)
    Z = p['Z']
    f1, f2 = _members(p, ref)
    before = [e.sweep_update('ei', float(ref[j]), k=10, want_moments=True) for j, e in enumerate((f1, f2))]
    means = [e.sweep_update('mean', None, k=0, want_all=True)['acq'] for e in (f1, f2)]
    long = Engine.ehvi_batch(f1, f2, P, ref, nb)
    short = Engine.ehvi_batch(f1, f2, P, ref, 3)
    again = Engine.ehvi_batch(f1, f2, P, ref, nb)
    np.testing.assert_array_equal(long['sel_idx'], r['idx'])
    # prefix and repeat
    for key in ('sel_val', 'sel_idx', 'sel_y', 'sel_nfront'):
        assert _same_bits(short[key], long[key][:3]), key
        assert _same_bits(again[key], long[key]), key
    assert _same_bits(short['sel_s2'], np.ascontiguousarray(long['sel_s2'][:, :3])) and _same_bits(again['sel_s2'], long['sel_s2'])
    # the believed outcomes are the members' own means at the picks: the believer does not move them
    for c in range(2):
        assert _same_bits(long['sel_y'][:, c], means[c][long['sel_idx']])
    # handles and caches are as they were
    for j, (e, upd) in enumerate(zip((f1, f2), before)):
        assert e.sweep_cache_size() == len(Z)
        after = e.sweep_update('ei', float(ref[j]), k=10, want_moments=True)
        for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
            np.testing.assert_array_equal(upd[key], after[key])
    # every pick's value is the fold's on its own four moments over the raw points P + the believed outcomes before it: the device's
    # insertion and its value, pinned without a tolerance
    for j in range(nb):
        mom = np.array([[long['sel_y'][j, 0]], [long['sel_s2'][0, j]], [long['sel_y'][j, 1]], [long['sel_s2'][1, j]]])
        raw = np.vstack([np.asarray(P, dtype=float).reshape(-1, 2), long['sel_y'][:j]])
        dmom = _dev(mom)
        one = f1.ehvi_fold(dmom.data_ptr(), 1, raw, ref, k=1)
        assert one['top_idx'][0] == 0 and one['top_val'][0] == long['sel_val'][j], (j, one['top_val'][0], long['sel_val'][j])
    # round 0 is the two-objective sweep's winner over the same candidates (LAST: it re-seeds the caches), for this front and for none
    for front in (P, None):
        first = Engine.ehvi_batch(f1, f2, front, ref, 1)
        full = Engine.ehvi_sweep(f1, f2, front, ref, Z, k=1, want_all=True)
        assert first['sel_idx'][0] == full['top_idx'][0] and first['sel_val'][0] == full['top_val'][0] == full['acq'][full['top_idx'][0]]
        assert first['sel_nfront'][0] == (0 if front is None else r['n'][0])
    _close([f1, f2])


def test_optional_outputs_may_be_null():
    from pybo_amd import _lib
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case('se_d8_stair16')
    f1, f2 = _members(p, ref)
    full = _lib.Engine.ehvi_batch(f1, f2, P, ref, nb)
    Pc, rc = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    sv, si = np.empty(nb), np.empty(nb, dtype=np.int64)
    assert f1._lib.gpx_ehvi_sweep_batch(f1._h, f2._h, _lib._ptr(Pc), len(Pc), _lib._ptr(rc), nb, _lib._ptr(sv), _lib._ptr(si), None, None, None) == 0
    assert _same_bits(sv, full['sel_val']) and _same_bits(si, full['sel_idx'])
    ny = np.empty(nb, dtype=np.int64)
    assert f1._lib.gpx_ehvi_sweep_batch(f1._h, f2._h, _lib._ptr(Pc), len(Pc), _lib._ptr(rc), nb, _lib._ptr(sv), _lib._ptr(si), None, None, _lib._ptr(ny)) == 0
    assert _same_bits(ny, full['sel_nfront']) and ny.tolist() == r['n'].tolist()
    _close([f1, f2])


# ---- 3. the grid-stride loop ------------------------------------------------------------------------------------------------------------
def test_the_grid_stride_path_beyond_262144_candidates():
    """batch_blocks caps the scoring launch at 1024 blocks of 256: with M > 262 144 every thread takes a second candidate.  262 144
    copies of NON-picked rows in front of the case's candidates can never win a round (the pick is strictly better; a copy ties only
    with its original), so the picks are the case's, shifted, and everything else is the plain run's bits."""
    from pybo_amd._lib import Engine
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case('m5_d6_stair16')
    Z = p['Z']
    rest = np.setdiff1d(np.arange(len(Z)), r['idx'])
    nfill = 262144
    Zbig = np.vstack([Z[rest[np.arange(nfill) % len(rest)]], Z])
    engines = _members(p, ref)
    plain = Engine.ehvi_batch(*engines, P, ref, nb)
    _close(engines)
    engines = _members(p, ref, Zbig)
    big = Engine.ehvi_batch(*engines, P, ref, nb)
    _close(engines)
    np.testing.assert_array_equal(plain['sel_idx'], r['idx'])
    np.testing.assert_array_equal(big['sel_idx'], nfill + r['idx'])
    for key in ('sel_val', 'sel_s2', 'sel_y', 'sel_nfront'):
        assert _same_bits(big[key], plain[key]), key


# ---- 4. queued appends ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['se_d8_means_n257', 'm5_d6_means_n257'])
def test_queued_corrections_are_flushed_first(tag):
    """Both members: fit N = 254, fill the cache, append 3 points WITHOUT re-scoring (their corrections wait in the member's queue, its
    factor crosses the 256-row block boundary), then pick: the reference has 257 observations, and so has its front."""
    from pybo_amd._lib import Engine
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case(tag)
    assert n_obs == 257
    engines = _members(p, ref, n=254)
    for j, e in enumerate(engines):
        for i in range(254, 257):
            assert e.append(p['X'][i], p['Y'][i, j])
    got = Engine.ehvi_batch(*engines, P, ref, nb)
    _close(engines)
    _check_against(p, r, got)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def _bind(path):
    from pybo_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def test_arguments_and_state_are_refused_alike_by_both_libraries():
    from pybo_amd import _lib
    p = ehvi_cases.build(100, 2, 'se', 5, m=40)
    X = np.ascontiguousarray(p['X'])
    cols = [np.ascontiguousarray(c) for c in p['Y'].T]
    ells = [np.ascontiguousarray(h[2]) for h in p['hypers']]
    rng = np.random.RandomState(0)
    Z, Z30, Zother = np.ascontiguousarray(p['Z']), np.ascontiguousarray(rng.rand(30, 2)), np.ascontiguousarray(rng.rand(40, 2))
    front = np.ascontiguousarray(p['Y'][:20])
    ref = np.ascontiguousarray(p['Y'].min(0) - 0.5)
    stair, sref = ehvi_cases.raw_front(1021, 3, lo=0.0, hi=1.0)
    stair, sref = np.ascontiguousarray(stair), np.ascontiguousarray(sref)
    stair1025 = np.ascontiguousarray(ehvi_cases.raw_front(1025, 4, lo=0.0, hi=1.0)[0])
    P = _lib._ptr
    codes = {}
    for name in ('libgpx.so', 'libgpx_diag.so'):
        lib = _bind(os.path.join(ROOT, 'pybo_amd', 'csrc', name))
        assert lib.gpx_version() >= 730
        hs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]           # the two objectives and a handle that is never fitted
        for h in hs:
            assert lib.gpx_create(0, None, C.byref(h)) == 0
        for h, y, l in zip(hs[:2], cols, ells):
            assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(l), 1.0, 1e-3, 0.0) == 0
        par = np.array([0.0])
        sv, si, s2, sy, sn = np.empty(64), np.empty(64, dtype=np.int64), np.empty(2 * 64), np.empty(2 * 64), np.empty(64, dtype=np.int64)
        tv, ti = np.empty(1), np.empty(1, dtype=np.int64)
        got = []

        def cache(h, Zc):
            assert lib.gpx_set_option(h, b'sweep_cache', 1) == 0
            assert lib.gpx_sweep(h, 0, P(par), 1, P(Zc), len(Zc), 1, P(tv), P(ti), None, None, None) == 0
            assert lib.gpx_set_option(h, b'sweep_cache', 0) == 0

        def call(nb=4, f1=hs[0], f2=hs[1], pts=front, np_=None, rf=ref, v=sv, i=si):
            rc = lib.gpx_ehvi_sweep_batch(f1, f2, P(pts) if pts is not None else None, (len(pts) if pts is not None else 0) if np_ is None else np_,
                                          P(rf) if rf is not None else None, nb, P(v), P(i), P(s2), P(sy), P(sn))
            msg = lib.gpx_last_error(f1) or b''
            assert rc == 0 or f1 is None or len(msg) > 0
            got.append(rc)
            return msg

        cache(hs[0], Z)
        msg = call()                                             # objective 2 has no cache yet: the message names it
        assert got[-1] == _lib.GPX_ESTATE and b'objective 2' in msg
        cache(hs[1], Z30)
        call()                                                   # caches of different sizes
        cache(hs[1], Zother)
        call()                                                   # equal sizes, different rows
        assert got[1:] == [_lib.GPX_EARG] * 2
        cache(hs[1], Z)
        call()                                                   # the first good call
        assert got[-1] == 0
        good = (sv[:4].copy(), si[:4].copy(), s2[:8].copy(), sy[:8].copy(), sn[:4].copy())
        mark = len(got)
        call(f1=None)                                            # NULL handles
        call(f2=None)
        call(f2=hs[0])                                           # the same handle twice
        call(pts=np.array([[0.0, np.nan]]))                      # a front that is not finite
        call(pts=np.array([[np.inf, 0.0]]))
        call(rf=np.array([0.0, np.nan]))                         # a reference point that is not finite
        call(rf=None)
        call(pts=None, np_=3)                                    # NULL front with np > 0
        call(np_=-1)                                             # np out of range
        call(pts=np.zeros((4097, 2)))
        call(pts=stair1025, rf=sref)                             # more than 1024 points on the front
        call(pts=stair, rf=sref, nb=5)                           # 1021 + 5 - 1 = 1025: the front could outgrow its arrays
        call(nb=0)
        call(nb=65)
        call(nb=41)                                              # nb > M
        call(v=None)                                             # NULL outputs
        call(i=None)
        assert got[mark:] == [_lib.GPX_EARG] * 17
        call(f2=hs[2])                                           # not fitted
        assert got[-1] == _lib.GPX_ESTATE
        # a refused call leaves nothing behind: the caches are live and the same call returns the same bits
        assert [lib.gpx_sweep_cache_size(h) for h in hs[:2]] == [40, 40]
        call()
        assert got[-1] == 0 and all(np.array_equal(a, b) for a, b in zip((sv[:4], si[:4], s2[:8], sy[:8], sn[:4]), good))
        call(pts=stair, rf=sref, nb=4)                           # 1021 + 4 - 1 = 1024: the cap, exactly
        assert got[-1] == 0 and sn[0] == 1021
        call(pts=None)                                           # np = 0: an empty front
        assert got[-1] == 0 and sn[0] == 0
        call(nb=40)                                              # nb = M: every candidate, each once
        assert got[-1] == 0 and sorted(si[:40].tolist()) == list(range(40))
        assert lib.gpx_fit(hs[1], P(X), 100, 2, P(cols[1]), 0, P(ells[1]), 1.0, 1e-3, 0.0) == 0
        msg = call()                                             # objective 2 refitted: its cache is gone
        assert got[-1] == _lib.GPX_ESTATE and b'objective 2' in msg
        cache(hs[1], Z)
        assert lib.gpx_fit(hs[0], P(X), 100, 2, P(cols[0]), 0, P(ells[0]), 1.0, 1e-3, 0.0) == 0
        msg = call()
        assert got[-1] == _lib.GPX_ESTATE and b'objective 1' in msg
        codes[name] = got
        for h in hs:
            assert lib.gpx_destroy(h) == 0
    assert codes['libgpx.so'] == codes['libgpx_diag.so']


# ---- 6. plug-in -------------------------------------------------------------------------------------------------------------------------
def _device_model(p):
    from pybo_amd import models
    model = models.MultiObjective(*[models.make_gp(sn2, rho, ell, bias, kernel=p['kernels'][j]) for j, (sn2, rho, ell, bias) in enumerate(p['hypers'])])
    model.add_data(p['X'], p['Y'])
    return model


def test_propose_batch_on_device_members_is_the_one_call_on_their_engines():
    import pybo_amd
    from pybo_amd import policies
    from pybo_amd._lib import DeviceGrid, Engine
    p = ehvi_cases.problem('se_d8', m=8)
    model = _device_model(p)
    bounds = np.array([[0.0, 1.0]] * p['d'])
    grid = DeviceGrid('uniform', bounds, 3001, seed=5)
    host_grid = np.asarray(grid)
    index = policies.EHVI(model, None, p['X'])
    front, ref = index.acq[1]
    assert index.acq[0] == 'ehvi' and not hasattr(index, 'batch')
    Xq, vals, idx = pybo_amd.propose_batch(model, bounds, p['X'], 8, policy=lambda m, b, x: index, xgrid=grid)
    engines = [m._engine() for m in model.objectives]
    assert engines[0].timers()['batch'] > 0 and all(m._state.cache_grid is grid for m in model.objectives)
    cold = [e.timers()['sweep_trmm'] for e in engines]
    assert all(t > 0 for t in cold)
    Xq2, vals2, idx2 = pybo_amd.propose_batch(model, bounds, p['X'], 8, policy=lambda m, b, x: index, xgrid=grid)
    assert [e.timers()['sweep_trmm'] for e in engines] == cold      # the second call only re-used the caches: no cold sweep
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(vals, vals2)
    np.testing.assert_array_equal(Xq, host_grid[idx])
    direct = Engine.ehvi_batch(engines[0], engines[1], front, ref, 8)
    np.testing.assert_array_equal(idx, direct['sel_idx'])
    np.testing.assert_array_equal(vals, direct['sel_val'])
    assert len(set(idx.tolist())) == 8
    # the policy by its name, and a host array (one copy for both members), pick the same rows
    Xq3, vals3, idx3 = pybo_amd.propose_batch(model, bounds, p['X'], 8, policy='ehvi', xgrid=host_grid)
    np.testing.assert_array_equal(idx3, idx)
    np.testing.assert_array_equal(vals3, vals)
    with pytest.raises(ValueError, match='two-objective'):
        pybo_amd.propose_batch(model, bounds, p['X'], 8, policy='ehvi', xgrid=grid, fantasies=4)
    grid.close()


def test_the_loop_in_batches_on_a_two_objective_device_model():
    import pybo_amd
    from pybo_amd import models
    from pybo_amd._lib import DeviceGrid
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    model = models.MultiObjective(models.make_gp(1e-4, 1.0, [0.4, 0.4], -0.3), models.make_gp(1e-4, 1.0, [0.4, 0.4], -0.3))
    grid = DeviceGrid('uniform', bounds, 2000, seed=2)

    def objective(x):
        x = np.ravel(x)
        return float(-np.sum((x - 0.2) ** 2)), float(-np.sum((x - 0.8) ** 2))

    xbest, model, info = pybo_amd.solve_bayesopt(objective, bounds, model=model, niter=12, policy='ehvi', recommender='pareto', nbatch=4,
                                                 batch_grid=grid, rng=0)
    assert model.ndata == 1 + 12 and len(info.x) == 13 and info.y.shape == (13, 2) and len(info.xbest) == 12
    host_grid = np.asarray(grid)
    assert all(any(np.array_equal(x, z) for z in host_grid) for x in info.x[1:])      # every evaluation after the seed is a grid point
    assert sum(m._engine().timers()['batch'] for m in model.objectives) > 0            # the device path
    grid.close()
