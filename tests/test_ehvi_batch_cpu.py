"""Batch proposals on a two-objective model, the parts that need no GPU: (a) the reference itself
(tests/ehvi_batch_ref.py): every case is admitted -- distinct picks, margins, separated coordinates -- and the size of the front that scored
each pick is the recorded sequence; (b) pybo_amd.propose_batch with policy='ehvi' on a models.MultiObjective of ORACLE members -- the
generic host path of pybo_amd/batch.py, both members observing each pick at their own posterior mean and the front growing by that row --
against the from-scratch greedy; (c) solve_bayesopt(nbatch=) on oracle members; (d) the refusals that come before any index is built;
(e) the EHVI index still carries no `.batch`; (f) the library exports gpx_ehvi_sweep_batch.

Tolerance of (b): the one the device is held to (ehvi_batch_ref.val_tol).  Both sides are the oracle's float64 arithmetic of the same
formula on the same data and agree far better -- they differ in that the host path predicts a pick alone where the reference reads it out
of the prediction of all of Z, and in pareto.py's EI against ehvi_ref.py's -- but the picks are compared exactly."""
import numpy as np
import pytest

import batch_ref
import ehvi_batch_ref
import ehvi_cases
import ehvi_ref
from oracle import gp_ref
import pybo_amd
from pybo_amd import models, policies


def _oracle_model(p, n=None):
    n = len(p['X']) if n is None else n
    model = models.MultiObjective(*[gp_ref.make_gp(*p['hypers'][j], p['kernels'][j]) for j in range(2)])
    model.add_data(p['X'][:n], p['Y'][:n])
    return model


# ---- (a) the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(ehvi_batch_ref.CASES))
def test_every_case_is_admitted_and_its_front_follows_the_recorded_sizes(tag):
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case(tag)
    print(tag, 'n', r['n'].tolist(), 'margin %.3g' % r['margin'].min(), 'separation / mu_tol %.1f' % ehvi_batch_ref.separation(p, r))
    assert batch_ref.MIN_MARGIN == 1e-5
    assert len(set(r['idx'].tolist())) == nb == len(r['idx'])
    assert np.all(r['margin'] >= batch_ref.MIN_MARGIN)
    assert ehvi_batch_ref.separation(p, r) >= 10.0
    assert ehvi_batch_ref.admitted(p, r)
    assert r['n'].tolist() == ehvi_batch_ref.N_PER_ROUND[tag]
    assert r['n'][0] + nb - 1 <= 1024 and len(P) <= 4096                   # what the device entry takes
    # a believed outcome is the members' means at the pick, and the front of round j + 1 is the front of P + the first j + 1 of them
    assert np.array_equal(r['y'], r['mom'][:, [0, 2]])
    for j in (1, nb - 1):
        a, b = ehvi_batch_ref.strips_vec(np.vstack([P, r['y'][:j]]), ref)
        assert np.array_equal(a, r['strips'][j][0]) and np.array_equal(b, r['strips'][j][1])      # (the tolerance's twin of ehvi_ref.strips)
    assert np.all(ehvi_batch_ref.val_tol(p, r) > 0)


def test_the_cases_exercise_removal_growth_and_no_change():
    steps = {t: np.diff(ehvi_batch_ref.N_PER_ROUND[t]) for t in ehvi_batch_ref.CASES}
    assert min(s.min() for s in steps.values()) <= -900                    # one pick dominates 900 points of a staircase
    assert all((s == 0).all() for t, s in steps.items() if t.endswith('highref'))
    assert any((s == 1).sum() >= 4 for s in steps.values())
    assert ehvi_batch_ref.N_PER_ROUND['se_d8_stair1021'][0] + 4 - 1 == 1024      # the cap, exactly


# ---- (b) the host path ---------------------------------------------------------------------------------------------------------------
def _check_host_path(tag, policy):
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case(tag)
    model = _oracle_model(p, n_obs)
    before = [(m.X.copy(), m.Y.copy()) for m in model.objectives]
    Xq, vals, idx = pybo_amd.propose_batch(model, np.array([[0.0, 1.0]] * p['d']), p['X'][:n_obs], nb, policy=policy, xgrid=p['Z'])
    tol = ehvi_batch_ref.val_tol(p, r)
    print('idx', idx, r['idx'])
    print('val err / tol', np.abs(vals - r['val']) / tol)
    assert ehvi_batch_ref.admitted(p, r)                                   # the admission condition, on the reference itself
    np.testing.assert_array_equal(idx, r['idx'])
    assert np.all(np.abs(vals - r['val']) <= tol)
    np.testing.assert_array_equal(Xq, p['Z'][idx])
    assert model.ndata == n_obs and all(np.array_equal(m.X, X0) and np.array_equal(m.Y, Y0) for m, (X0, Y0) in zip(model.objectives, before))
    v0 = model.get_ehvi(P, ref, p['Z'])                                    # round 0 is the index's own best grid point
    assert idx[0] == gp_ref.topk_desc(v0, 1)[0] and vals[0] == v0[idx[0]]


def test_propose_batch_on_oracle_members_equals_the_from_scratch_greedy():
    """'ehvi' with the policy's own front and reference point: the posterior means at X over F.min(0) - 0.1 span, the case 'means'."""
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case('m5_d6_means')
    index = policies.EHVI(_oracle_model(p), None, p['X'])
    assert np.array_equal(index.acq[1][0], P) and np.array_equal(index.acq[1][1], ref)
    _check_host_path('m5_d6_means', 'ehvi')


def test_propose_batch_with_a_reference_point_nothing_reaches():
    """ref above every posterior mean: no believed outcome enters the front, every round is the product of the two EIs over ref -- the
    front in the policy's hands (the means at X) lies below ref and is filtered away, as the case's empty one."""
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case('se_d8_highref')
    _check_host_path('se_d8_highref', ('ehvi', dict(ref=ref)))


def test_both_members_observe_a_pick_at_their_own_mean_and_the_front_grows_by_that_row():
    p = ehvi_cases.build(60, 3, 'se', 4, m=300)
    model = _oracle_model(p)
    seen, fronts = [], []

    class Spy(models.MultiObjective):
        def copy(self):
            return Spy(*[m.copy() for m in self.objectives])

        def add_data(self, X, Y):
            seen.append((np.array(X), np.array(Y), [float(m.predict(X)[0][0]) for m in self.objectives]))
            models.MultiObjective.add_data(self, X, Y)

        def get_ehvi(self, front, ref, X, grad=False):
            fronts.append(np.array(front))
            return models.MultiObjective.get_ehvi(self, front, ref, X, grad)

    spy = Spy(*[m.copy() for m in model.objectives])
    Xq, vals, idx = pybo_amd.propose_batch(spy, np.array([[0.0, 1.0]] * 3), p['X'], 4, policy='ehvi', xgrid=p['Z'])
    assert len(seen) == 3                                                  # nb - 1 believer steps, none after the last pick
    for (x, y, means), i in zip(seen, idx):
        assert np.array_equal(x, p['Z'][i:i + 1]) and y.shape == (1, 2) and np.array_equal(y[0], means)
    grown = [f for f in fronts if len(f) >= 60][-4:]                       # the four rounds' fronts (the spy's copies score them)
    assert [len(f) for f in grown] == [60, 61, 62, 63]
    for j in range(1, 4):
        assert np.array_equal(grown[j][:-1], grown[j - 1]) and np.array_equal(grown[j][-1], seen[j - 1][1][0])
    assert len(set(idx.tolist())) == 4


# ---- (c) the loop ----------------------------------------------------------------------------------------------------------------------
def test_solve_bayesopt_in_batches_on_oracle_members():
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    model = models.MultiObjective(gp_ref.make_gp(1e-4, 1.0, [0.4, 0.4], -0.3), gp_ref.make_gp(1e-4, 1.0, [0.4, 0.4], -0.3))
    grid = np.random.RandomState(2).rand(300, 2)

    def objective(x):
        x = np.ravel(x)
        return float(-np.sum((x - 0.2) ** 2)), float(-np.sum((x - 0.8) ** 2))

    xbest, model, info = pybo_amd.solve_bayesopt(objective, bounds, model=model, niter=8, policy='ehvi', recommender='pareto', nbatch=4,
                                                 batch_grid=grid, rng=0)
    assert model.ndata == 1 + 8 and len(info.x) == 9 and info.y.shape == (9, 2) and len(info.xbest) == 8
    assert all(any(np.array_equal(x, z) for z in grid) for x in info.x[1:])      # every evaluation after the seed is a grid point
    assert len({tuple(x) for x in info.x[1:5]}) == 4                              # a batch's picks are distinct


# ---- (d) refusals ----------------------------------------------------------------------------------------------------------------------
def test_fantasies_and_pending_are_refused_before_an_index_is_built():
    p = ehvi_cases.build(40, 3, 'se', 4, m=100)
    model = _oracle_model(p)
    bounds = np.array([[0.0, 1.0]] * 3)
    built = []

    def policy(model, bounds, X):
        built.append(1)
        return policies.EHVI(model, bounds, X)

    for kw in (dict(fantasies=8), dict(pending=[3]), dict(fantasies=8, pending=[3])):
        with pytest.raises(ValueError, match='two-objective'):
            pybo_amd.propose_batch(model, bounds, p['X'], 4, policy=policy, xgrid=p['Z'], **kw)
    assert built == []
    pybo_amd.propose_batch(model, bounds, p['X'], 2, policy=policy, xgrid=p['Z'])
    assert built == [1]


# ---- (e), (f) ----------------------------------------------------------------------------------------------------------------------------
def test_the_ehvi_index_still_has_no_batch_and_other_models_are_refused_by_name():
    p = ehvi_cases.build(40, 3, 'se', 4, m=100)
    model = _oracle_model(p)
    index = policies.EHVI(model, None, p['X'])
    assert index.acq[0] == 'ehvi' and not hasattr(index, 'batch')
    from pybo_amd.batch import _score
    with pytest.raises(ValueError, match='batch proposals need an EI, PI or UCB index'):
        _score(model.objectives[0], 'ehvi', index.acq[1], p['Z'])                # a single model has no get_ehvi
    assert np.array_equal(_score(model, 'ehvi', index.acq[1], p['Z']), index(p['Z']))
    assert not hasattr(_oracle_model(p), '_lead') and callable(models.MultiObjective.acq_batch)
    with pytest.raises(ValueError, match="takes 'ehvi'"):
        model.acq_batch('ei', index.acq[1], p['Z'], 2)
    with pytest.raises(TypeError, match='device GP members'):
        model.acq_batch('ehvi', index.acq[1], p['Z'], 2)                         # oracle members: the host path is batch.py's


def test_the_library_exports_the_entry():
    from pybo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, 'gpx_ehvi_sweep_batch') and 'gpx_ehvi_sweep_batch' in _lib.SYMBOLS and lib.gpx_version() >= 730
    assert len(_lib.SYMBOLS['gpx_ehvi_sweep_batch'][1]) == 11 and callable(_lib.Engine.ehvi_batch)
