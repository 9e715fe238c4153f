"""gpx_ensemble_sweep_batch on the device: nb greedy picks of the ensemble's EI / PI / UCB on the members' live sweep caches, the
members frozen and each conditioned on a pick at its own posterior mean, against the from-scratch greedy of
tests/ens_batch_ref.py.  Shapes as in test_gpu_batch.py (N off and on the tiles, M = 3001 over many blocks) plus d = 260 (the pick
kernel's gather beyond one step of 256 threads) and M > 262 144 (the scoring kernel's grid-stride loop)."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_ref
import ens_batch_ref
from helpers import synth_problem, s2_tol, mu_tol, branin
from test_gpu_batch import acq_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _member(X, y, kernel, hyp, Z, kind='ei', param=0.4):
    """A fitted engine with the hyper-parameters hyp = (ell, rho, sn2, bias) whose sweep cache holds Z."""
    from pybo_amd._lib import Engine
    ell, rho, sn2, bias = hyp
    e = Engine(0)
    e.fit(X, y, kernel, ell, rho, sn2, bias)
    e.set_option('sweep_cache', 1)
    e.sweep(kind, param, Z, k=1, want_all=False)
    e.set_option('sweep_cache', 0)
    return e


def _members(prob, Z=None):
    Z = prob['Z'] if Z is None else Z
    return [_member(prob['X'], prob['y'], prob['kernel'], hyp, Z, prob['kind'], prob['param']) for hyp in prob['hypers']]


def _close(engines):
    for e in engines:
        e.close()


def val_tol(kind, param, hypers, mu, s2):
    """The stated moment tolerances of every member propagated to first order through the ensemble's value, at the reference's
    member moments mu, s2 (n, nb).  EI / PI: the mean over the members of test_gpu_batch.acq_tol.  UCB: with dmu = mean_m mu_tol_m
    and ds2 = mean_m(s2_tol_m + 2 |mu_m| mu_tol_m) + 2 |mu| dmu (s2 = mean(s2_m + mu_m^2) - mu^2), 1e-6 |v| + 1.05 (dmu +
    sqrt(beta) / (2 s) ds2)."""
    rhos = np.array([h[1] for h in hypers])[:, None]
    if kind != 'ucb':
        return np.mean([acq_tol(kind, param, mu[m], s2[m], rhos[m, 0]) for m in range(len(hypers))], axis=0)
    mut, s2t = mu_tol(mu, rhos), s2_tol(s2, rhos)
    mix_mu = mu.mean(axis=0)
    mix_s2 = np.maximum((s2 + mu ** 2).mean(axis=0) - mix_mu ** 2, 0.0)
    dmu = mut.mean(axis=0)
    ds2 = (s2t + 2.0 * np.abs(mu) * mut).mean(axis=0) + 2.0 * np.abs(mix_mu) * dmu
    s = np.sqrt(mix_s2)
    return 1e-6 * np.abs(mix_mu + np.sqrt(param * mix_s2)) + 1.05 * (dmu + np.sqrt(param) / (2.0 * s) * ds2)


def _check_against(prob, ref, got):
    hypers, kind, param = prob['hypers'], prob['kind'], prob['param']
    rhos = np.array([h[1] for h in hypers])[:, None]
    print('margins', ref['margin'])
    print('idx', got['sel_idx'], ref['idx'])
    print('val err / tol', np.abs(got['sel_val'] - ref['val']) / val_tol(kind, param, hypers, ref['mu'], ref['s2']))
    print('s2 err / tol', (np.abs(got['sel_s2'] - ref['s2']) / s2_tol(ref['s2'], rhos)).max(axis=1))
    assert ens_batch_ref.admitted(ref)                                # the admission condition, on the reference itself
    np.testing.assert_array_equal(got['sel_idx'], ref['idx'])
    assert got['sel_s2'].shape == ref['s2'].shape
    assert np.all(np.abs(got['sel_s2'] - ref['s2']) <= s2_tol(ref['s2'], rhos))
    assert np.all(np.abs(got['sel_val'] - ref['val']) <= val_tol(kind, param, hypers, ref['mu'], ref['s2']))


@pytest.mark.parametrize('tag', sorted(ens_batch_ref.CASES))
def test_picks_values_and_member_variances_equal_the_from_scratch_greedy(tag):
    from pybo_amd._lib import Engine
    prob, ref = ens_batch_ref.case(tag)
    engines = _members(prob)
    got = Engine.ensemble_batch(engines, prob['kind'], prob['param'], prob['nb'])
    _close(engines)
    _check_against(prob, ref, got)


@pytest.mark.parametrize('tag', ['se_300_3_ei', 'matern1_130_5_pi'])
def test_one_member_gives_the_single_handle_batch_bit_for_bit(tag):
    from pybo_amd._lib import Engine
    prob, _ = batch_ref.case(tag)
    e = _member(prob['X'], prob['y'], prob['kernel'], (prob['ell'], prob['rho'], prob['sn2'], prob['bias']), prob['Z'])
    one = e.sweep_batch(prob['kind'], prob['param'], prob['nb'])
    ens = Engine.ensemble_batch([e], prob['kind'], prob['param'], prob['nb'])
    again = e.sweep_batch(prob['kind'], prob['param'], prob['nb'])
    e.close()
    for got in (ens, again):
        np.testing.assert_array_equal(got['sel_idx'], one['sel_idx'])
        np.testing.assert_array_equal(got['sel_val'], one['sel_val'])
        np.testing.assert_array_equal(np.ravel(got['sel_s2']), one['sel_s2'])


def test_round_zero_prefixes_and_repeats_are_bit_identical():
    from pybo_amd._lib import Engine
    prob, ref = ens_batch_ref.case('se_300_3_ei_n3')
    engines = _members(prob)
    # round 0 is the ensemble sweep's winner over the same candidates, value and index, for every acquisition
    for kind, param in (('ei', prob['param']), ('pi', prob['param'] + 0.05), ('ucb', 2.0)):
        full = Engine.ensemble_sweep(engines, kind, param, prob['Z'], k=1)
        first = Engine.ensemble_batch(engines, kind, param, 1)
        assert first['sel_idx'][0] == full['top_idx'][0] and first['sel_val'][0] == full['top_val'][0], kind
        assert first['sel_val'][0] == full['acq'][full['top_idx'][0]]
    kind, param = prob['kind'], prob['param']
    long = Engine.ensemble_batch(engines, kind, param, 8)
    short = Engine.ensemble_batch(engines, kind, param, 3)
    again = Engine.ensemble_batch(engines, kind, param, 8)
    _close(engines)
    np.testing.assert_array_equal(long['sel_idx'], ref['idx'])
    for key in ('sel_val', 'sel_idx'):
        np.testing.assert_array_equal(short[key], long[key][:3])
        np.testing.assert_array_equal(again[key], long[key])
    np.testing.assert_array_equal(short['sel_s2'], long['sel_s2'][:, :3])
    np.testing.assert_array_equal(again['sel_s2'], long['sel_s2'])


def test_no_member_is_disturbed():
    from pybo_amd._lib import Engine
    prob, _ = ens_batch_ref.case('matern3_200_20_ei_n3')
    kind, param = prob['kind'], prob['param']
    engines = _members(prob)
    before = [(e.sweep_update(kind, param, k=10, want_moments=True), e.get_matrix('L'), e.get_vectors()) for e in engines]
    Engine.ensemble_batch(engines, kind, param, 8)
    for e, (upd, L0, (a0, al0)) in zip(engines, before):
        after = e.sweep_update(kind, param, k=10, want_moments=True)
        for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
            np.testing.assert_array_equal(upd[key], after[key])
        np.testing.assert_array_equal(e.get_matrix('L'), L0)
        np.testing.assert_array_equal(e.get_vectors()[0], a0)
        np.testing.assert_array_equal(e.get_vectors()[1], al0)
    _close(engines)


def test_a_members_live_announcement_survives():
    from pybo_amd._lib import Engine
    X, y, ell = synth_problem(300, 3, seed=12)
    Z = np.random.RandomState(1).rand(5000, 3)
    hypers = ens_batch_ref.member_hypers(ell, 2)
    xn, yn = np.array([0.31, 0.62, 0.47]), 0.25
    outs = []
    for with_batch in (True, False):
        engines = [_member(X, y, 'matern5', hyp, Z) for hyp in hypers]
        e = engines[1]
        assert e.append_begin(xn)
        if with_batch:
            picks = Engine.ensemble_batch(engines, 'ei', 0.4, 5)
            assert len(set(picks['sel_idx'].tolist())) == 5
        assert e.append(xn, yn)
        r = e.sweep_update('ei', 0.4, k=5, want_moments=True)
        outs.append((r, e.get_matrix('L'), e.get_vectors()[1]))
        _close(engines)
    for key in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        np.testing.assert_array_equal(outs[0][0][key], outs[1][0][key])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def test_queued_corrections_are_flushed_first():
    """Every member: fit N = 254, fill the cache, append 3 points WITHOUT re-scoring (their corrections wait in the member's queue,
    its factor crosses the 256-row block boundary), then pick: the reference has 257 observations."""
    from pybo_amd._lib import Engine
    kernel, d = 'matern5', 3
    X, y, ell = synth_problem(257, d, seed=17)
    Z = np.random.RandomState(5).rand(3001, d)
    hypers = ens_batch_ref.member_hypers(ell, 2)
    target = ens_batch_ref.ensemble_param(X, y, kernel, hypers, 'ei')
    prob = dict(hypers=hypers, kind='ei', param=target)
    ref = ens_batch_ref.greedy(X, y, Z, kernel, hypers, 'ei', target, 8)
    engines = [_member(X[:254], y[:254], kernel, hyp, Z) for hyp in hypers]
    for e in engines:
        for i in range(254, 257):
            assert e.append(X[i], y[i])
    got = Engine.ensemble_batch(engines, 'ei', target, 8)
    _close(engines)
    _check_against(prob, ref, got)


def test_the_grid_stride_path_beyond_262144_candidates():
    """batch_blocks caps the scoring launch at 1024 blocks of 256: with M > 262 144 every thread takes a second candidate.  262 144
    copies of NON-picked rows in front of the case's candidates can never win a round (the pick is strictly better; a copy ties
    only with its original), so the picks are the case's, shifted, and values and variances are the plain run's bits."""
    from pybo_amd._lib import Engine
    prob, ref = ens_batch_ref.case('se_300_3_ei_n3')
    Z = prob['Z']
    rest = np.setdiff1d(np.arange(len(Z)), ref['idx'])
    nfill = 262144
    Zbig = np.vstack([Z[rest[np.arange(nfill) % len(rest)]], Z])
    engines = _members(prob)
    plain = Engine.ensemble_batch(engines, prob['kind'], prob['param'], prob['nb'])
    _close(engines)
    engines = _members(prob, Zbig)
    big = Engine.ensemble_batch(engines, prob['kind'], prob['param'], prob['nb'])
    _close(engines)
    np.testing.assert_array_equal(plain['sel_idx'], ref['idx'])
    np.testing.assert_array_equal(big['sel_idx'], nfill + ref['idx'])
    np.testing.assert_array_equal(big['sel_val'], plain['sel_val'])
    np.testing.assert_array_equal(big['sel_s2'], plain['sel_s2'])


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
    ell2 = np.ascontiguousarray(ell * 1.2)
    rng = np.random.RandomState(0)
    Z, Z30, Zother = (np.ascontiguousarray(rng.rand(m, 2)) for m in (40, 30, 40))
    P = _lib._ptr
    codes = {}
    for name in ('libgpx.so', 'libgpx_diag.so'):
        lib = _bind(os.path.join(ROOT, 'pybo_amd', 'csrc', name))
        hs = [C.c_void_p(), C.c_void_p()]
        for h, l in zip(hs, (ell, ell2)):
            assert lib.gpx_create(0, None, C.byref(h)) == 0
            assert lib.gpx_fit(h, P(X), 100, 2, P(y), 0, P(l), 1.0, 1e-3, 0.0) == 0
        par = np.array([0.3])
        sv, si, s2 = np.empty(64), np.empty(64, dtype=np.int64), np.empty(128)
        tv, ti = np.empty(1), np.empty(1, dtype=np.int64)
        got = []

        def cache(h, Zc):
            assert lib.gpx_set_option(h, b'sweep_cache', 1) == 0
            assert lib.gpx_sweep(h, 0, P(par), 1, P(Zc), len(Zc), 1, P(tv), P(ti), None, None, None) == 0
            assert lib.gpx_set_option(h, b'sweep_cache', 0) == 0

        def call(acq, params, nparams, nb, v, i, members=None, n=2):
            members = hs if members is None else members
            arr = (C.c_void_p * max(len(members), 1))(*[m.value for m in members])
            rc = lib.gpx_ensemble_sweep_batch(arr, n, acq, params, nparams, nb, v, i, P(s2))
            msg = lib.gpx_last_error(members[0]) or b''
            assert rc == 0 or len(msg) > 0
            got.append(rc)
            return msg

        cache(hs[0], Z)
        msg = call(0, P(par), 1, 4, P(sv), P(si))                # member 1 has no cache yet: the message names it
        assert got[-1] == _lib.GPX_ESTATE and b'member 1' in msg
        cache(hs[1], Z30)
        call(0, P(par), 1, 4, P(sv), P(si))                      # caches of different sizes
        cache(hs[1], Zother)
        call(0, P(par), 1, 4, P(sv), P(si))                      # equal sizes, different rows
        cache(hs[1], Z)
        call(0, P(par), 1, 4, P(sv), P(si), [hs[0], hs[0]])      # a handle listed twice
        call(3, None, 0, 4, P(sv), P(si))                        # GPX_ACQ_MEAN
        call(0, P(par), 1, 0, P(sv), P(si))                      # nb = 0
        call(0, P(par), 1, 65, P(sv), P(si))                     # nb = 65
        call(0, P(par), 1, 41, P(sv), P(si))                     # nb > M
        call(0, P(par), 1, 4, None, P(si))                       # NULL outputs
        call(0, P(par), 1, 4, P(sv), None)
        call(0, None, 0, 4, P(sv), P(si))                        # no parameter
        call(0, P(par), 1, 4, P(sv), P(si), n=0)                 # n_members = 0
        call(0, P(par), 1, 4, P(sv), P(si), [hs[0]] * 65, n=65)  # n_members = 65
        assert got[1:] == [_lib.GPX_EARG] * 12
        call(0, P(par), 1, 40, P(sv), P(si))                     # nb = M: every candidate, each once
        assert got[-1] == 0 and sorted(si[:40].tolist()) == list(range(40))
        assert lib.gpx_fit(hs[1], P(X), 100, 2, P(y), 0, P(ell2), 1.0, 1e-3, 0.0) == 0
        call(0, P(par), 1, 4, P(sv), P(si))                      # one member refitted: its cache is gone
        assert got[-1] == _lib.GPX_ESTATE
        codes[name] = got
        for h in hs:
            assert lib.gpx_destroy(h) == 0
    assert codes['libgpx.so'] == codes['libgpx_diag.so']


BRANIN_BOUNDS = np.array([[-5.0, 10.0], [0.0, 15.0]])


def _branin_mcmc():
    """models.MCMC(n = 3) over the device GP on the Branin data of test_gpu_batch.py."""
    from pybo_amd import models
    bounds = BRANIN_BOUNDS
    rng = np.random.RandomState(0)
    X = bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * rng.rand(400, 2)
    y = -branin(X) / 10.0
    hyp = (1e-4 * np.var(y), np.var(y), 0.25 * (bounds[:, 1] - bounds[:, 0]), np.mean(y))
    gp = models.make_gp(*hyp)
    gp.params['like.sn2'].set_prior('lognormal', np.log(hyp[0]), 1.0)
    gp.params['kern.rho'].set_prior('lognormal', np.log(hyp[1]), 1.0)
    gp.params['kern.ell'].set_prior('uniform', 0.01 * np.ones(2), 15.0 * np.ones(2))
    gp.params['mean.bias'].set_prior('normal', hyp[3], hyp[1])
    gp.add_data(X, y)
    return X, y, models.MCMC(gp, n=3, burn=5, rng=0)


def test_propose_batch_on_the_default_model_takes_the_device_path():
    """The plug-in level: propose_batch over models.MCMC with device members takes the device path, re-uses the members' live
    caches, and picks what the from-scratch greedy picks with the sampled hyper-parameters held fixed."""
    import pybo_amd
    from pybo_amd import inits
    bounds = BRANIN_BOUNDS
    X, y, mc = _branin_mcmc()
    grid = inits.init_sobol_device(bounds, 30000, rng=3)
    host_grid = np.asarray(grid)

    Xq, vals, idx = pybo_amd.propose_batch(mc, bounds, X, 8, policy='ei', xgrid=grid)
    engines = mc._engines()
    tm = engines[0].timers()
    assert tm['batch'] > 0 and all(m._state.cache_grid is grid for m in mc._members)
    launches = [e.timers()['sweep_trmm_launches'] for e in engines]
    Xq2, vals2, idx2 = pybo_amd.propose_batch(mc, bounds, X, 8, policy='ei', xgrid=grid)
    assert [e.timers()['sweep_trmm_launches'] for e in engines] == launches      # the second call only re-used the caches
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(vals, vals2)
    np.testing.assert_array_equal(Xq, host_grid[idx])

    th = mc.samples                                       # [log sn2, log rho, log ell.., bias] per member
    hypers = [(np.exp(t[2:4]), float(np.exp(t[1])), float(np.exp(t[0])), float(t[4])) for t in th]
    target = float(mc.predict_mean(X).max())
    ref = ens_batch_ref.greedy(X, y, host_grid, 'se', hypers, 'ei', target, 8)
    print('margins', ref['margin'])
    assert ens_batch_ref.admitted(ref)
    np.testing.assert_array_equal(idx, ref['idx'])
    err = np.abs(vals - ref['val']) / val_tol('ei', target, hypers, ref['mu'], ref['s2'])
    print('val err / tol', err)
    assert np.all(err <= 1.0)


def test_the_loop_in_batches_on_the_default_model():
    import pybo_amd
    from pybo_amd import inits
    X, y, mc = _branin_mcmc()
    grid = inits.init_sobol_device(BRANIN_BOUNDS, 30000, rng=3)
    xb, model, info = pybo_amd.solve_bayesopt(lambda x: float(-branin(x)[0] / 10.0), BRANIN_BOUNDS, model=mc, niter=8, policy='ei',
                                              recommender='incumbent', nbatch=4, batch_grid=grid, rng=1)
    assert model.ndata == 400 + 1 + 8 and len(info.x) == 9
    assert model._members[0]._engine().timers()['batch'] > 0        # the batches went through the device path
