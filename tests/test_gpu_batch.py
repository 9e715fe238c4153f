"""gpx_sweep_batch on the device: nb greedy picks on the live sweep cache, each conditioned on the earlier ones at their posterior
mean, against the from-scratch greedy of tests/batch_ref.py (refit on [X; picks] with believer values every round).  The cases
(batch_ref.CASES) put N off the 64-row tile (300, 130, 140), on a 128-block multiple (256), M = 3001 off every tile and over
many blocks, d below and above the 16-coordinate staging chunk."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.special import erfc

import batch_ref
from oracle import gp_ref
from helpers import synth_problem, s2_tol, mu_tol, ei_tol, branin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(X, y, kernel, ell, rho, sn2, bias, Z, kind='ei', param=0.4):
    """A fitted engine whose sweep cache holds Z."""
    from pybo_amd._lib import Engine
    e = Engine(0)
    e.fit(X, y, kernel, ell, rho, sn2, bias)
    e.set_option('sweep_cache', 1)
    e.sweep(kind, param, Z, k=1, want_all=False)
    e.set_option('sweep_cache', 0)
    return e


def _case_engine(tag):
    prob, ref = batch_ref.case(tag)
    e = _engine(prob['X'], prob['y'], prob['kernel'], prob['ell'], prob['rho'], prob['sn2'], prob['bias'], prob['Z'], prob['kind'],
                prob['param'])
    return prob, ref, e


def acq_tol(kind, param, mu, s2, rho):
    """The stated moment tolerances (helpers.mu_tol / s2_tol) propagated to first order through the acquisition, plus 1e-6
    relative -- helpers.ei_tol's construction for PI = Phi(z), z = (mu - t) / s (dPI/dmu = phi(z) / s, dPI/ds2 = -phi(z) z / (2 s2))
    and UCB = mu + sqrt(beta s2) (dUCB/dmu = 1, dUCB/ds2 = sqrt(beta) / (2 s))."""
    if kind == 'ei':
        return ei_tol(mu, s2, param, rho)
    s = np.sqrt(s2)
    if kind == 'ucb':
        return 1e-6 * np.abs(mu + np.sqrt(param * s2)) + 1.05 * (mu_tol(mu, rho) + np.sqrt(param) / (2.0 * s) * s2_tol(s2, rho))
    z = (mu - param) / s
    cdf = 0.5 * erfc(-z * 0.70710678118654752440)
    pdf = 0.39894228040143267794 * np.exp(-0.5 * z * z)
    return 1e-6 * np.abs(cdf) + 1.05 * (pdf / s * mu_tol(mu, rho) + pdf * np.abs(z) / (2.0 * s2) * s2_tol(s2, rho))


def _check_against(ref, got, kind, param, rho, upto=None):
    n = len(ref['idx']) if upto is None else upto
    print('margins', ref['margin'][:n])
    print('idx', got['sel_idx'][:n], ref['idx'][:n])
    print('val err / tol', np.abs(got['sel_val'][:n] - ref['val'][:n]) / acq_tol(kind, param, ref['mu_pick'][:n], ref['s2'][:n], rho))
    print('s2 err / tol', np.abs(got['sel_s2'][:n] - ref['s2'][:n]) / s2_tol(ref['s2'][:n], rho))
    assert ref['margin'][:n].min() >= batch_ref.MIN_MARGIN            # the admission condition, on the reference itself
    np.testing.assert_array_equal(got['sel_idx'][:n], ref['idx'][:n])
    assert np.all(np.abs(got['sel_s2'][:n] - ref['s2'][:n]) <= s2_tol(ref['s2'][:n], rho))
    assert np.all(np.abs(got['sel_val'][:n] - ref['val'][:n]) <= acq_tol(kind, param, ref['mu_pick'][:n], ref['s2'][:n], rho))


@pytest.mark.parametrize('tag', sorted(batch_ref.CASES))
def test_picks_values_and_variances_equal_the_from_scratch_greedy(tag):
    prob, ref, e = _case_engine(tag)
    got = e.sweep_batch(prob['kind'], prob['param'], prob['nb'], want_s2_all=True)
    e.close()
    assert len(set(ref['idx'].tolist())) == prob['nb']
    _check_against(ref, got, prob['kind'], prob['param'], prob['rho'])
    # the variances that scored the last pick: conditioned on the first nb - 1 picks, on EVERY candidate
    err = np.abs(got['s2_all'] - ref['s2_last']) / s2_tol(ref['s2_last'], prob['rho'])
    print('s2_all worst err / tol', err.max())
    assert np.all(err <= 1.0)


def test_nothing_is_disturbed_and_results_repeat():
    prob, ref, e = _case_engine('matern3_200_20_ei')
    kind, param = prob['kind'], prob['param']
    before = e.sweep_update(kind, param, k=10, want_moments=True)
    L0, (a0, al0) = e.get_matrix('L'), e.get_vectors()
    first = e.sweep_batch(kind, param, 8, want_s2_all=True)
    after = e.sweep_update(kind, param, k=10, want_moments=True)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        np.testing.assert_array_equal(before[key], after[key])
    np.testing.assert_array_equal(e.get_matrix('L'), L0)
    np.testing.assert_array_equal(e.get_vectors()[0], a0)
    np.testing.assert_array_equal(e.get_vectors()[1], al0)
    again = e.sweep_batch(kind, param, 8, want_s2_all=True)
    for key in ('sel_val', 'sel_idx', 'sel_s2', 's2_all'):
        np.testing.assert_array_equal(first[key], again[key])
    short = e.sweep_batch(kind, param, 3)
    for key in ('sel_val', 'sel_idx', 'sel_s2'):
        np.testing.assert_array_equal(short[key], first[key][:3])
    # round 0 is the plain re-scoring's winner, bit for bit
    assert first['sel_idx'][0] == before['top_idx'][0] and first['sel_val'][0] == before['top_val'][0]
    assert first['sel_s2'][0] == before['s2'][before['top_idx'][0]]
    e.close()


def test_queued_corrections_are_flushed_first():
    """Fit N = 254, fill the cache, append 3 points WITHOUT re-scoring (their corrections wait in the queue, the factor crosses
    the 256-row block boundary), then pick: the reference has 257 observations."""
    kernel, d, rho, sn2, bias = 'matern5', 3, 1.3, 1e-3, 0.2
    X, y, ell = synth_problem(257, d, seed=17)
    Z = np.random.RandomState(5).rand(3001, d)
    base = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    base.add_data(X, y)
    target = float(base.mean_at_obs().max())
    ref = batch_ref.greedy(X, y, Z, kernel, ell, rho, sn2, bias, 'ei', target, 8)
    e = _engine(X[:254], y[:254], kernel, ell, rho, sn2, bias, Z)
    for i in range(254, 257):
        assert e.append(X[i], y[i])
    got = e.sweep_batch('ei', target, 8)
    _check_against(ref, got, 'ei', target, rho)
    # ... and the flushed sums are the ones a re-scoring now reads
    upd = e.sweep_update('ei', target, k=1, want_moments=True)
    assert upd['top_idx'][0] == got['sel_idx'][0] and upd['top_val'][0] == got['sel_val'][0]
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
            picks = e.sweep_batch('ei', 0.4, 5)
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
        h = C.c_void_p()
        assert lib.gpx_create(0, None, C.byref(h)) == 0
        assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(ell), 1.0, 1e-3, 0.0) == 0
        par = np.array([0.3])
        sv, si, s2 = np.empty(64), np.empty(64, dtype=np.int64), np.empty(64)
        got = []

        def call(acq, params, nparams, nb, v, i):
            rc = lib.gpx_sweep_batch(h, acq, params, nparams, nb, v, i, P(s2), None)
            msg = lib.gpx_last_error(h) or b''
            assert rc == 0 or len(msg) > 0
            got.append(rc)

        call(0, P(par), 1, 4, P(sv), P(si))                      # no cache yet
        assert got[-1] == _lib.GPX_ESTATE
        tv, ti = np.empty(1), np.empty(1, dtype=np.int64)
        assert lib.gpx_set_option(h, b'sweep_cache', 1) == 0
        assert lib.gpx_sweep(h, 0, P(par), 1, P(Z), 40, 1, P(tv), P(ti), None, None, None) == 0
        assert lib.gpx_set_option(h, b'sweep_cache', 0) == 0
        call(3, None, 0, 4, P(sv), P(si))                        # GPX_ACQ_MEAN
        call(0, P(par), 1, 0, P(sv), P(si))                      # nb = 0
        call(0, P(par), 1, 65, P(sv), P(si))                     # nb = 65
        call(0, P(par), 1, 41, P(sv), P(si))                     # nb > M
        call(0, P(par), 1, 4, None, P(si))                       # NULL outputs
        call(0, P(par), 1, 4, P(sv), None)
        call(0, None, 0, 4, P(sv), P(si))                        # no parameter
        assert got[1:] == [_lib.GPX_EARG] * 7
        call(0, P(par), 1, 40, P(sv), P(si))                     # nb = M: every candidate, each once
        assert got[-1] == 0 and sorted(si[:40].tolist()) == list(range(40))
        assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(ell), 1.0, 1e-3, 0.0) == 0
        call(0, P(par), 1, 4, P(sv), P(si))                      # a refit dropped the cache
        assert got[-1] == _lib.GPX_ESTATE
        codes[name] = got
        assert lib.gpx_destroy(h) == 0
    assert codes['libgpx.so'] == codes['libgpx_diag.so']


def test_propose_batch_and_the_loop_on_a_device_grid(monkeypatch):
    """The plug-in level on the Branin problem of test_gpu_warm.py: propose_batch over models.GP takes the device path and re-uses
    a live cache; its picks are those of the generic host path over the oracle's model on the same grid."""
    import pybo_amd
    from pybo_amd import models, inits
    bounds = np.array([[-5.0, 10.0], [0.0, 15.0]])
    rng = np.random.RandomState(0)
    X = bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * rng.rand(400, 2)
    y = -branin(X) / 10.0
    hyp = (1e-4 * np.var(y), np.var(y), 0.25 * (bounds[:, 1] - bounds[:, 0]), np.mean(y))
    gp = models.make_gp(*hyp)
    gp.add_data(X, y)
    ref = gp_ref.make_gp(*hyp)
    ref.add_data(X, y)
    grid = inits.init_sobol_device(bounds, 30000, rng=3)
    host_grid = np.asarray(grid)

    Xq, vals, idx = pybo_amd.propose_batch(gp, bounds, X, 8, policy='ei', xgrid=grid)
    eng = gp._engine()
    tm = eng.timers()
    assert tm['batch'] > 0 and gp._state.cache_grid is grid
    launches = tm['sweep_trmm_launches']
    Xq2, vals2, idx2 = pybo_amd.propose_batch(gp, bounds, X, 8, policy='ei', xgrid=grid)
    assert eng.timers()['sweep_trmm_launches'] == launches          # the second call only re-used the cache
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(vals, vals2)
    np.testing.assert_array_equal(Xq, host_grid[idx])

    # the generic host path over the oracle's model, its per-round scores recorded for the margin condition
    from pybo_amd import batch
    rounds, score = [], batch._score
    monkeypatch.setattr(batch, '_score', lambda *a: rounds.append(score(*a)) or rounds[-1])
    Xr, vr, ir = pybo_amd.propose_batch(ref, bounds, X, 8, policy='ei', xgrid=host_grid)
    monkeypatch.undo()
    margins = []
    for j, v in enumerate(rounds):
        v = v.copy()
        v[ir[:j]] = -np.inf
        second = np.partition(v, -2)[-2]
        margins.append((v[ir[j]] - second) / abs(v[ir[j]]))
    print('margins', margins)
    assert len(margins) == 8 and min(margins) >= batch_ref.MIN_MARGIN
    np.testing.assert_array_equal(idx, ir)
    target = float(ref.predict(X)[0].max())
    mu_p, s2_p = ref.predict(host_grid[ir[:1]])                     # round 0's moments: the tolerance of its value
    assert abs(vals[0] - vr[0]) <= ei_tol(mu_p, s2_p, target, hyp[1])[0]

    xb, model, info = pybo_amd.solve_bayesopt(lambda x: float(-branin(x)[0] / 10.0), bounds, model=gp, niter=12, policy='ei',
                                              recommender='incumbent', nbatch=4, batch_grid=grid, rng=1)
    assert model.ndata == 400 + 1 + 12 and len(info.x) == 13
    assert model._state.cache_grid is grid                          # batches of <= 16 rows extend the factor in place: the cache lives on
