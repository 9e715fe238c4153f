"""gpx_sweep_batch_fantasy on the device: greedy batch picks on the live sweep cache with the pending outcomes integrated out over S joint
fantasies, against tests/fant_ref.py -- greedy_refits (every round refits [X; picks] with every fantasy's own sampled observations;
nothing of the recurrence) on the four admitted cases, greedy_recurrence where 64 refits would be too slow.  The cases put N off the
64-row tile (300, 130, 200) and on a 128-block multiple (256), M = 3001 off every tile and over many workgroups, d below and above the
16-coordinate staging chunk, S on (16, 64), below (8) and off (5) the scoring kernel's chunk of 16 fantasies."""
import ctypes as C
import os

import numpy as np
import pytest

import fant_ref
from oracle import gp_ref
from helpers import synth_problem, s2_tol, branin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = sorted(fant_ref.CASES)
KEYS = ('sel_val', 'sel_idx', 'sel_s2', 's2_all')


def _engine(X, y, kernel, ell, rho, sn2, bias, Z, kind='ei', param=0.4):
    """A fitted engine whose sweep cache holds Z."""
    from pybo_amd._lib import Engine
    e = Engine(0)
    e.fit(X, y, kernel, ell, rho, sn2, bias)
    e.set_option('sweep_cache', 1)
    e.sweep(kind, param, Z, k=1, want_all=False)
    e.set_option('sweep_cache', 0)
    return e


def _prob_engine(prob):
    return _engine(prob['X'], prob['y'], prob['kernel'], prob['ell'], prob['rho'], prob['sn2'], prob['bias'], prob['Z'], prob['kind'],
                   prob['param'])


def _check_against(prob, ref, got, incumbent, eps=None, upto=None, picks=None):
    """Picks over the leading `picks` rounds, values and variances over the leading `upto` (default: all)."""
    eps = prob['eps'] if eps is None else eps
    n = len(ref['idx']) if upto is None else upto
    k = n if picks is None else picks
    tol = np.array([fant_ref.value_tol(prob['kind'], ref, eps, prob['rho'], j, incumbent) for j in range(n)])
    print('margins', ref['margin'][:n])
    print('idx', got['sel_idx'][:n], ref['idx'][:n])
    with np.errstate(invalid='ignore'):                               # (a forced row's EI may be exactly 0: 0 / 0)
        print('val err / tol', np.abs(got['sel_val'][:n] - ref['val'][:n]) / tol)
    print('s2 err / tol', np.abs(got['sel_s2'][:n] - ref['s2'][:n]) / s2_tol(ref['s2'][:n], prob['rho']))
    assert ref['margin'][:k].min() >= fant_ref.MIN_MARGIN             # the admission condition, on the reference itself
    np.testing.assert_array_equal(got['sel_idx'][:k], ref['idx'][:k])
    assert np.all(np.abs(got['sel_s2'][:n] - ref['s2'][:n]) <= s2_tol(ref['s2'][:n], prob['rho']))
    assert np.all(np.abs(got['sel_val'][:n] - ref['val'][:n]) <= tol)


@pytest.mark.parametrize('incumbent', [0, 1])
@pytest.mark.parametrize('tag', CASE_IDS)
def test_picks_values_and_variances_equal_the_from_scratch_refits(tag, incumbent):
    prob, ref = fant_ref.case(tag, incumbent)
    e = _prob_engine(prob)
    got = e.sweep_batch_fantasy(prob['kind'], prob['param'], prob['nb'], prob['eps'], incumbent=incumbent, want_s2_all=True)
    e.close()
    assert len(set(ref['idx'].tolist())) == prob['nb']
    _check_against(prob, ref, got, incumbent)
    # the variances that scored the last pick: conditioned on the first nb - 1 picks, on EVERY candidate
    err = np.abs(got['s2_all'] - ref['s2_last']) / s2_tol(ref['s2_last'], prob['rho'])
    print('s2_all worst err / tol', err.max())
    assert np.all(err <= 1.0)


@pytest.mark.parametrize('tag', ['matern3_200_20_ei_s5', 'matern5_256_2_pi_s8'])
def test_one_fantasy_of_zeros_is_the_believer_bit_for_bit(tag):
    prob, _ = fant_ref.case(tag, 0)
    e = _prob_engine(prob)
    want = e.sweep_batch(prob['kind'], prob['param'], prob['nb'], want_s2_all=True)
    for ld in (prob['nb'] - 1, 63):
        got = e.sweep_batch_fantasy(prob['kind'], prob['param'], prob['nb'], np.zeros((1, ld)), incumbent=0, want_s2_all=True)
        for key in KEYS:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    again = e.sweep_batch(prob['kind'], prob['param'], prob['nb'], want_s2_all=True)      # ... and leaves the believer's call as it was
    e.close()
    for key in KEYS:
        np.testing.assert_array_equal(again[key], want[key], err_msg=key)


@pytest.mark.parametrize('incumbent', [0, 1])
def test_sixty_four_fantasies_and_sixty_four_picks(incumbent):
    """The extremes of both loops: 63 rows of V under 64 running means in four chunks (32 KB of innovations in LDS), against the
    recurrence in numpy.  eps seed 23 admits all 64 rounds in both modes (the smallest margins 5.2e-4 / 1.1e-4); the test asks for 16."""
    prob = fant_ref.problem('matern1_130_5_ei_s64')
    ref = fant_ref.run(fant_ref.greedy_recurrence, prob, incumbent, nb=64)
    low = np.nonzero(ref['margin'] < fant_ref.MIN_MARGIN)[0]
    lead = int(low[0]) if len(low) else 64
    print('admitted leading rounds', lead)
    assert lead >= 16
    e = _prob_engine(prob)
    got = e.sweep_batch_fantasy(prob['kind'], prob['param'], 64, prob['eps'], incumbent=incumbent, want_s2_all=True)
    e.close()
    assert len(set(got['sel_idx'].tolist())) == 64
    differ = np.nonzero(got['sel_idx'] != ref['idx'])[0]
    same = int(differ[0]) if len(differ) else 64                     # values and variances at the reference's own picks: up to there
    assert same >= lead
    _check_against(prob, ref, got, incumbent, upto=same, picks=lead)
    if same == 64:
        assert np.all(np.abs(got['s2_all'] - ref['s2_last']) <= s2_tol(ref['s2_last'], prob['rho']))


def test_a_short_batch_is_a_prefix_and_results_repeat():
    prob, _ = fant_ref.case('matern3_200_20_ei_s5', 1)
    e = _prob_engine(prob)
    kind, param, eps = prob['kind'], prob['param'], prob['eps']
    eps16 = fant_ref.eps_for(16)
    eps16[:5] = eps                                                   # 16 fantasies whose leading five are the case's
    for incumbent in (0, 1):
        full = e.sweep_batch_fantasy(kind, param, 8, eps, incumbent=incumbent, want_s2_all=True)
        short = e.sweep_batch_fantasy(kind, param, 3, eps, incumbent=incumbent)
        for key in KEYS[:3]:
            np.testing.assert_array_equal(short[key], full[key][:3], err_msg=key)
        again = e.sweep_batch_fantasy(kind, param, 8, eps, incumbent=incumbent, want_s2_all=True)
        for key in KEYS:
            np.testing.assert_array_equal(again[key], full[key], err_msg=key)
        # a narrower copy of the same normals (another ld_eps) is the same call
        narrow = e.sweep_batch_fantasy(kind, param, 8, np.ascontiguousarray(eps[:, :7]), incumbent=incumbent, want_s2_all=True)
        for key in KEYS:
            np.testing.assert_array_equal(narrow[key], full[key], err_msg=key)
        # eleven more fantasies change the values (sanity: S is not ignored beyond the first chunk's live part) ...
        wide = e.sweep_batch_fantasy(kind, param, 8, eps16, incumbent=incumbent, want_s2_all=True)
        assert wide['sel_idx'][0] == full['sel_idx'][0] and not np.array_equal(wide['sel_val'][1:], full['sel_val'][1:])
        # ... and repeat, too
        wide2 = e.sweep_batch_fantasy(kind, param, 8, eps16, incumbent=incumbent, want_s2_all=True)
        for key in KEYS:
            np.testing.assert_array_equal(wide2[key], wide[key], err_msg=key)
    e.close()


def test_pending_rows_are_forced_and_integrated_over():
    from pybo_amd import _lib
    prob, ref = fant_ref.case('se_300_3_ei_s16', 1)
    e = _prob_engine(prob)
    kind, param, eps, nb = prob['kind'], prob['param'], prob['eps'], prob['nb']
    free = e.sweep_batch_fantasy(kind, param, nb, eps, incumbent=1, want_s2_all=True)
    forced = e.sweep_batch_fantasy(kind, param, nb, eps, incumbent=1, pending=free['sel_idx'][:2], want_s2_all=True)
    for key in KEYS:
        np.testing.assert_array_equal(forced[key], free[key], err_msg=key)
    pend = [1500, 7, 2999]                                           # rows of three different workgroups, none of them a free pick
    assert not set(pend) & set(ref['idx'].tolist())
    for incumbent in (0, 1):
        want = fant_ref.run(fant_ref.greedy_recurrence, prob, incumbent, pending=pend)
        assert np.all(np.isinf(want['margin'][:3])) and want['margin'][3:].min() >= fant_ref.MIN_MARGIN
        got = e.sweep_batch_fantasy(kind, param, nb, eps, incumbent=incumbent, pending=pend, want_s2_all=True)
        assert got['sel_idx'][:3].tolist() == pend
        _check_against(prob, want, got, incumbent)
        assert np.all(np.abs(got['s2_all'] - want['s2_last']) <= s2_tol(want['s2_last'], prob['rho']))
    for bad in ([7, 7], [7, 1500, 7], [-1], [3001], list(range(nb)), list(range(nb + 1))):
        with pytest.raises(_lib.GpxError) as err:
            e.sweep_batch_fantasy(kind, param, nb, eps, pending=bad)
        assert err.value.code == _lib.GPX_EARG, bad
    after = e.sweep_batch_fantasy(kind, param, nb, eps, incumbent=1, want_s2_all=True)      # a refused call leaves nothing behind
    e.close()
    for key in KEYS:
        np.testing.assert_array_equal(after[key], free[key], err_msg=key)


def test_nothing_is_disturbed():
    prob, _ = fant_ref.case('matern3_200_20_ei_s5', 1)
    e = _prob_engine(prob)
    kind, param = prob['kind'], prob['param']
    before = e.sweep_update(kind, param, k=10, want_moments=True)
    L0, (a0, al0) = e.get_matrix('L'), e.get_vectors()
    first = e.sweep_batch_fantasy(kind, param, 6, prob['eps'], want_s2_all=True)
    after = e.sweep_update(kind, param, k=10, want_moments=True)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        np.testing.assert_array_equal(before[key], after[key])
    np.testing.assert_array_equal(e.get_matrix('L'), L0)
    np.testing.assert_array_equal(e.get_vectors()[0], a0)
    np.testing.assert_array_equal(e.get_vectors()[1], al0)
    # round 0 has nothing pending: the plain re-scoring's winner (its value summed five times and divided by five: to a few ulp)
    assert first['sel_idx'][0] == before['top_idx'][0] and abs(first['sel_val'][0] - before['top_val'][0]) <= 1e-14 * before['top_val'][0]
    assert first['sel_s2'][0] == before['s2'][before['top_idx'][0]]
    assert e.timers()['batch'] > 0
    e.close()


def test_queued_corrections_are_flushed_first():
    """Fit N = 254, fill the cache, append 3 points WITHOUT re-scoring (their corrections wait in the queue, the factor crosses the 256-row
    block boundary), then pick: the reference has 257 observations."""
    kernel, d, rho, sn2, bias, S, nb = 'matern5', 3, 1.3, 1e-3, 0.2, 8, 6
    X, y, ell = synth_problem(257, d, seed=17)
    Z = np.random.RandomState(5).rand(3001, d)
    base = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    base.add_data(X, y)
    target = float(base.mean_at_obs().max())
    prob = dict(X=X, y=y, ell=ell, Z=Z, kernel=kernel, kind='ei', param=target, nb=nb, S=S, eps=fant_ref.eps_for(S), rho=rho, sn2=sn2, bias=bias)
    ref = fant_ref.run(fant_ref.greedy_recurrence, prob, 1)
    e = _engine(X[:254], y[:254], kernel, ell, rho, sn2, bias, Z)
    for i in range(254, 257):
        assert e.append(X[i], y[i])
    got = e.sweep_batch_fantasy('ei', target, nb, prob['eps'], incumbent=1)
    _check_against(prob, ref, got, 1)
    upd = e.sweep_update('ei', target, k=1, want_moments=True)       # ... and the flushed sums are the ones a re-scoring now reads
    assert upd['top_idx'][0] == got['sel_idx'][0] and abs(upd['top_val'][0] - got['sel_val'][0]) <= 1e-14 * upd['top_val'][0]
    e.close()


def test_a_live_announcement_survives():
    X, y, ell = synth_problem(300, 3, seed=12)
    rho, sn2, bias = 1.3, 1e-3, 0.2
    Z = np.random.RandomState(1).rand(5000, 3)
    xn, yn = np.array([0.31, 0.62, 0.47]), 0.25
    outs = []
    for with_batch in (True, False):
        e = _engine(X, y, 'matern5', ell, rho, sn2, bias, Z)
        assert e.append_begin(xn)
        if with_batch:
            picks = e.sweep_batch_fantasy('ei', 0.4, 5, fant_ref.eps_for(8))
            assert len(set(picks['sel_idx'].tolist())) == 5
        assert e.append(xn, yn)
        r = e.sweep_update('ei', 0.4, k=5, want_moments=True)
        outs.append((r, e.get_matrix('L'), e.get_vectors()[1]))
        e.close()
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        np.testing.assert_array_equal(outs[0][0][key], outs[1][0][key])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def _bind(path):
    from pybo_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def test_arguments_and_state_are_refused_alike_by_both_libraries():
    from pybo_amd import _lib
    X, y, ell = synth_problem(100, 2, seed=1)
    X, y, ell = np.ascontiguousarray(X), np.ascontiguousarray(y), np.ascontiguousarray(ell)
    Z = np.ascontiguousarray(np.random.RandomState(0).rand(40, 2))
    P = _lib._ptr
    codes = {}
    for name in ('libgpx.so', 'libgpx_diag.so'):
        lib = _bind(os.path.join(ROOT, 'pybo_amd', 'csrc', name))
        assert lib.gpx_version() >= 710
        h = C.c_void_p()
        assert lib.gpx_create(0, None, C.byref(h)) == 0
        assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(ell), 1.0, 1e-3, 0.0) == 0
        par = np.array([0.3])
        eps = np.ascontiguousarray(np.random.RandomState(3).randn(64, 63))
        sv, si, s2 = np.empty(64), np.empty(64, dtype=np.int64), np.empty(64)
        pend = np.array([5, 9], dtype=np.int64)
        got = []

        def call(acq=0, params=P(par), nparams=1, nb=4, e=eps, S=8, ld=63, inc=1, pd=None, npd=0, v=P(sv), i=P(si)):
            rc = lib.gpx_sweep_batch_fantasy(h, acq, params, nparams, nb, None if e is None else P(e), S, ld, inc, pd, npd, v, i, P(s2), None)
            msg = lib.gpx_last_error(h) or b''
            assert rc == 0 or len(msg) > 0
            got.append(rc)

        call()                                                       # no cache yet
        assert got[-1] == _lib.GPX_ESTATE
        tv, ti = np.empty(1), np.empty(1, dtype=np.int64)
        assert lib.gpx_set_option(h, b'sweep_cache', 1) == 0
        assert lib.gpx_sweep(h, 0, P(par), 1, P(Z), 40, 1, P(tv), P(ti), None, None, None) == 0
        assert lib.gpx_set_option(h, b'sweep_cache', 0) == 0
        n0 = len(got)
        call(S=0), call(S=65), call(S=-1)
        bad = eps.copy()
        bad[3, 2] = np.nan
        call(e=bad)                                                  # a NaN inside the (S, nb - 1) block that is read
        bad[3, 2] = np.inf
        call(e=bad)
        call(e=None)
        call(ld=2)                                                   # ld_eps < nb - 1
        call(nb=1, ld=0)                                             # ... and < 1
        call(acq=2), call(acq=3, params=None, nparams=0), call(acq=16), call(acq=32)      # UCB, MEAN, MES, KG
        call(inc=2), call(inc=-1)
        call(nb=0), call(nb=65), call(nb=41), call(v=None), call(i=None), call(params=None, nparams=0)
        call(pd=P(pend), npd=4), call(pd=P(pend), npd=-1), call(pd=None, npd=1)
        assert got[n0:] == [_lib.GPX_EARG] * (len(got) - n0) and len(got) - n0 == 23
        ok = eps.copy()
        ok[3, 3] = np.nan                                            # outside the block nb = 4 reads: not looked at
        call(e=ok)
        assert got[-1] == 0
        call(nb=1, ld=1)                                             # one pick: nothing pending, no innovation read
        assert got[-1] == 0
        call(e=np.ascontiguousarray(eps[:, :3]), ld=3, pd=P(pend), npd=2)
        assert got[-1] == 0 and si[:2].tolist() == [5, 9]
        call(nb=40, S=64)                                            # nb = M: every candidate, each once
        assert got[-1] == 0 and sorted(si[:40].tolist()) == list(range(40))
        assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(ell), 1.0, 1e-3, 0.0) == 0
        call()                                                       # a refit dropped the cache
        assert got[-1] == _lib.GPX_ESTATE
        codes[name] = got
        assert lib.gpx_destroy(h) == 0
    assert codes['libgpx.so'] == codes['libgpx_diag.so']


def test_propose_batch_and_the_loop_on_a_device_grid():
    """The plug-in level: propose_batch over models.GP takes the device path on a DeviceGrid's live cache; its picks are those of the generic
    host path over the oracle's model on the same grid and normals, which are greedy_refits' (admitted on the reference's own margins)."""
    import pybo_amd
    from pybo_amd import models, inits
    from pybo_amd._lib import DeviceGrid
    bounds = np.array([[0.0, 1.0]] * 2)
    grid = inits.init_sobol_device(bounds, 3001, rng=3)
    assert isinstance(grid, DeviceGrid)
    prob = dict(fant_ref.problem('matern5_256_2_pi_s8'))
    prob['Z'] = np.asarray(grid)                                     # the case's model and normals on the device's own grid
    ref = fant_ref.run(fant_ref.greedy_refits, prob, 1)
    print('margins', ref['margin'])
    assert ref['margin'].min() >= fant_ref.MIN_MARGIN                # admitted (9.7e-3 on this grid)

    def frozen(model, bounds, X):                                    # the policies' own index, at the case's parameter
        from pybo_amd.policies.simple import _attach_topk
        return _attach_topk(lambda X, grad=False: model.get_tail(prob['param'], X, grad), model, 'pi', prob['param'])

    gp = models.make_gp(prob['sn2'], prob['rho'], prob['ell'], prob['bias'], kernel=prob['kernel'])
    gp.add_data(prob['X'], prob['y'])
    host = gp_ref.make_gp(prob['sn2'], prob['rho'], prob['ell'], prob['bias'], prob['kernel'])
    host.add_data(prob['X'], prob['y'])
    kw = dict(policy=frozen, rng=fant_ref.EPS_SEED, fantasies=8)
    Xq, vals, idx = pybo_amd.propose_batch(gp, bounds, prob['X'], prob['nb'], xgrid=grid, **kw)
    assert gp._engine().timers()['batch'] > 0 and gp._state.cache_grid is grid
    Xr, vr, ir = pybo_amd.propose_batch(host, bounds, prob['X'], prob['nb'], xgrid=prob['Z'], **kw)
    np.testing.assert_array_equal(ir, ref['idx'])
    np.testing.assert_array_equal(idx, ir)
    np.testing.assert_array_equal(Xq, prob['Z'][ir])
    tol = np.array([fant_ref.value_tol('pi', ref, prob['eps'], prob['rho'], j, 1) for j in range(prob['nb'])])
    print('val err / tol', np.abs(vals - vr) / tol)
    assert np.all(np.abs(vals - vr) <= tol)
    pend = [int(ir[0]), int(ir[1])]
    _, vals2, idx2 = pybo_amd.propose_batch(gp, bounds, prob['X'], prob['nb'], xgrid=grid, pending=pend, **kw)
    np.testing.assert_array_equal(idx2, idx)
    np.testing.assert_array_equal(vals2, vals)

    bb = np.array([[-5.0, 10.0], [0.0, 15.0]])
    rng = np.random.RandomState(0)
    X = bb[:, 0] + (bb[:, 1] - bb[:, 0]) * rng.rand(400, 2)
    y = -branin(X) / 10.0
    bgp = models.make_gp(1e-4 * np.var(y), np.var(y), 0.25 * (bb[:, 1] - bb[:, 0]), np.mean(y))
    bgp.add_data(X, y)
    bgrid = inits.init_sobol_device(bb, 30000, rng=3)
    xb, model, info = pybo_amd.solve_bayesopt(lambda x: float(-branin(x)[0] / 10.0), bb, model=bgp, niter=12, policy='ei',
                                              recommender='incumbent', nbatch=4, batch_grid=bgrid, batch_fantasies=8, rng=1)
    assert model.ndata == 400 + 1 + 12 and len(info.x) == 13 and len(info.xbest) == 12
    assert model._state.cache_grid is bgrid                          # batches of <= 16 rows extend the factor in place: the cache lives on
