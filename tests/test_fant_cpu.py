"""Fantasised batch proposals on the host (no GPU): the two references of tests/fant_ref.py against each other, the generic path of
pybo_amd.propose_batch(..., fantasies=S) over the oracle's GPRef against the from-scratch one, what fantasies = 0 leaves alone, and the
refusals."""
import numpy as np
import pytest

import fant_ref
from oracle import gp_ref
from helpers import loop_objective

import pybo_amd
from pybo_amd import models

CASE_IDS = sorted(fant_ref.CASES)


def _frozen(kind, param):
    """A policy whose index carries the case's own parameter (the policies derive theirs from the model)."""
    def policy(model, bounds, X):
        def index(X, grad=False):
            raise AssertionError('the batch path scores through the model protocol')
        index.acq = (kind, param)
        return index
    return policy


def _model(prob):
    gp = gp_ref.make_gp(prob['sn2'], prob['rho'], prob['ell'], prob['bias'], prob['kernel'])
    gp.add_data(prob['X'], prob['y'])
    return gp


@pytest.mark.parametrize('incumbent', [0, 1])
@pytest.mark.parametrize('tag', CASE_IDS)
def test_the_recurrence_equals_the_from_scratch_refits(tag, incumbent):
    prob, ref = fant_ref.case(tag, incumbent)
    _, rec = fant_ref.case_recurrence(tag, incumbent)
    print('margins', ref['margin'])
    assert ref['margin'].min() >= fant_ref.MIN_MARGIN and rec['margin'].min() >= fant_ref.MIN_MARGIN      # admitted, on the reference itself
    assert len(set(ref['idx'].tolist())) == prob['nb']
    np.testing.assert_array_equal(rec['idx'], ref['idx'])
    for key in ('val', 's2', 'mu_pick', 't', 'vrow', 'gain', 's2_last'):
        np.testing.assert_allclose(rec[key], ref[key], rtol=1e-9, atol=1e-9, err_msg=key)
    if incumbent:
        assert np.all(np.diff(ref['t'], axis=0) >= 0) and np.any(ref['t'][-1] > prob['param'])      # targets only rise, and some do
    else:
        assert np.all(ref['t'] == prob['param'])


@pytest.mark.parametrize('tag', CASE_IDS)
def test_the_fantasies_pick_differently_from_the_believer(tag):
    import batch_ref
    prob, ref = fant_ref.case(tag, 0)
    bel = batch_ref.greedy(prob['X'], prob['y'], prob['Z'], prob['kernel'], prob['ell'], prob['rho'], prob['sn2'], prob['bias'], prob['kind'],
                           prob['param'], prob['nb'])
    assert bel['idx'][0] == ref['idx'][0] and abs(bel['val'][0] - ref['val'][0]) <= 1e-12      # round 0: nothing is pending yet
    assert not np.array_equal(bel['idx'], ref['idx'])
    # one fantasy with zero innovations IS the believer
    one = fant_ref.run(fant_ref.greedy_refits, prob, 0, eps=np.zeros((1, fant_ref.EPS_COLS)))
    np.testing.assert_array_equal(one['idx'], bel['idx'])
    np.testing.assert_allclose(one['val'], bel['val'], rtol=1e-12)


@pytest.mark.parametrize('incumbent', ['fixed', 'fantasy'])
@pytest.mark.parametrize('tag', CASE_IDS)
def test_the_generic_host_path_equals_the_from_scratch_refits(tag, incumbent):
    prob, ref = fant_ref.case(tag, int(incumbent == 'fantasy'))
    assert ref['margin'].min() >= fant_ref.MIN_MARGIN
    gp = _model(prob)
    d = prob['X'].shape[1]
    Xq, vals, idx = pybo_amd.propose_batch(gp, [[0.0, 1.0]] * d, prob['X'], prob['nb'], policy=_frozen(prob['kind'], prob['param']),
                                           xgrid=prob['Z'], rng=fant_ref.EPS_SEED, fantasies=prob['S'], incumbent=incumbent)
    np.testing.assert_array_equal(idx, ref['idx'])
    np.testing.assert_array_equal(Xq, prob['Z'][ref['idx']])
    np.testing.assert_allclose(vals, ref['val'], rtol=1e-9, atol=1e-12)
    assert gp.ndata == len(prob['X'])                                 # the caller's model is left alone


def test_pending_rows_lead_the_batch_and_are_integrated_over():
    prob, ref = fant_ref.case('matern5_256_2_pi_s8', 1)
    gp = _model(prob)
    pend = [int(ref['idx'][0]), int(ref['idx'][1])]
    kw = dict(policy=_frozen(prob['kind'], prob['param']), xgrid=prob['Z'], rng=fant_ref.EPS_SEED, fantasies=prob['S'])
    _, vals, idx = pybo_amd.propose_batch(gp, [[0.0, 1.0]] * 2, prob['X'], prob['nb'], pending=pend, **kw)
    np.testing.assert_array_equal(idx, ref['idx'])                    # forcing a free run's own picks changes nothing
    np.testing.assert_allclose(vals, ref['val'], rtol=1e-9)
    other = [1500, 7]
    want = fant_ref.run(fant_ref.greedy_refits, prob, 1, pending=other)
    assert want['margin'].min() >= fant_ref.MIN_MARGIN and np.all(np.isinf(want['margin'][:2]))
    _, vals, idx = pybo_amd.propose_batch(gp, [[0.0, 1.0]] * 2, prob['X'], prob['nb'], pending=other, **kw)
    assert list(idx[:2]) == other
    np.testing.assert_array_equal(idx, want['idx'])
    np.testing.assert_allclose(vals, want['val'], rtol=1e-9)
    for bad in ([7, 7], [-1], [3001], list(range(prob['nb']))):
        with pytest.raises(ValueError, match='pending'):
            pybo_amd.propose_batch(gp, [[0.0, 1.0]] * 2, prob['X'], prob['nb'], pending=bad, **kw)
    with pytest.raises(ValueError, match='fantasies'):
        pybo_amd.propose_batch(gp, [[0.0, 1.0]] * 2, prob['X'], prob['nb'], policy=kw['policy'], xgrid=prob['Z'], pending=[7])


def test_zero_fantasies_leave_results_and_the_random_stream_alone():
    prob, _ = fant_ref.case('matern1_130_5_ei_s64', 0)
    gp = _model(prob)
    bounds = [[0.0, 1.0]] * 5
    outs, tails = [], []
    for kw in ({}, dict(fantasies=0), dict(fantasies=0, incumbent='fixed')):
        rng = np.random.RandomState(11)
        outs.append(pybo_amd.propose_batch(gp, bounds, prob['X'], 4, policy='ei', ngrid=500, rng=rng, **kw))      # the grid is drawn from rng
        tails.append(rng.rand(3))
    for out, tail in zip(outs[1:], tails[1:]):
        for a, b in zip(out, outs[0]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(tail, tails[0])
    # with fantasies the normals are drawn AFTER the grid: the same grid, (S, 63) normals further on in the stream
    rng = np.random.RandomState(11)
    Xq, _, idx = pybo_amd.propose_batch(gp, bounds, prob['X'], 4, policy='ei', ngrid=500, rng=rng, fantasies=3)
    twin = np.random.RandomState(11)
    grid = pybo_amd.inits.init_uniform(np.array(bounds), 500, twin)
    twin.randn(3, 63)
    np.testing.assert_array_equal(Xq, grid[idx])
    np.testing.assert_array_equal(rng.rand(3), twin.rand(3))
    assert idx[0] == outs[0][2][0]                                    # round 0 has nothing pending: the believer's first pick


class _Members(object):
    """What an ensemble looks like to propose_batch: the model protocol and `members`."""

    def __init__(self, gp):
        self._gp, self.members = gp, [gp]

    def copy(self):
        return _Members(self._gp.copy())

    def predict(self, X, grad=False):
        return self._gp.predict(X, grad)

    def get_improvement(self, target, X, grad=False):
        return self._gp.get_improvement(target, X, grad)


def test_what_is_not_built_is_refused_by_name():
    prob, _ = fant_ref.case('matern1_130_5_ei_s64', 0)
    gp = _model(prob)
    bounds, X, Z = [[0.0, 1.0]] * 5, prob['X'], prob['Z'][:300]
    with pytest.raises(ValueError, match='ensemble'):
        pybo_amd.propose_batch(_Members(gp), bounds, X, 3, policy='ei', xgrid=Z, fantasies=4)
    mc = models.MCMC(gp, n=2, burn=0, rng=0)
    assert hasattr(mc, 'members')
    with pytest.raises(ValueError, match='ensemble'):
        pybo_amd.propose_batch(mc, bounds, X, 3, policy=_frozen('ei', prob['param']), xgrid=Z, fantasies=4)
    sharded = object.__new__(models.ShardedGP)                       # (no device needed: the refusal comes before anything is asked of it)
    with pytest.raises(ValueError, match='ShardedGP'):
        pybo_amd.propose_batch(sharded, bounds, X, 3, policy=_frozen('ei', prob['param']), xgrid=Z, fantasies=4)
    with pytest.raises(ValueError, match='UCB'):
        pybo_amd.propose_batch(gp, bounds, X, 3, policy='ucb', xgrid=Z, fantasies=4)
    for kind in ('mes', 'kg'):
        with pytest.raises(ValueError, match='EI or PI'):
            pybo_amd.propose_batch(gp, bounds, X, 3, policy=_frozen(kind, np.array([1.0])), xgrid=Z, fantasies=4)
    with pytest.raises(ValueError, match='sampled'):
        pybo_amd.propose_batch(gp, bounds, X, 3, policy=('thompson', {'n': 20}), xgrid=Z, fantasies=4, rng=0)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match='fantasies'):
            pybo_amd.propose_batch(gp, bounds, X, 3, policy='ei', xgrid=Z, fantasies=bad)
    with pytest.raises(ValueError, match='incumbent'):
        pybo_amd.propose_batch(gp, bounds, X, 3, policy='ei', xgrid=Z, fantasies=4, incumbent='best y')
    # ... while the believer still serves all of them as before
    _, _, idx = pybo_amd.propose_batch(gp, bounds, X, 3, policy='ucb', xgrid=Z)
    assert len(set(idx.tolist())) == 3


def test_solve_bayesopt_forwards_the_fantasies(tmp_path):
    gp = gp_ref.make_gp(1e-4, 1.0, [0.3, 0.35], 0.0)
    X0 = np.random.RandomState(2).rand(6, 2)
    gp.add_data(X0, [loop_objective(x) for x in X0])
    grid = np.random.RandomState(7).rand(400, 2)
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    kw = dict(model=gp, niter=8, policy='ei', recommender='incumbent', nbatch=3, batch_grid=grid)
    _, model, info = pybo_amd.solve_bayesopt(loop_objective, bounds, rng=0, batch_fantasies=4, **kw)
    assert len(info.x) == 9 and model.ndata == 6 + 9
    assert len({tuple(x) for x in info.x}) == 9                       # no point twice
    _, _, again = pybo_amd.solve_bayesopt(loop_objective, bounds, rng=0, batch_fantasies=4, **kw)
    np.testing.assert_array_equal(info.x, again.x)
    _, _, plain = pybo_amd.solve_bayesopt(loop_objective, bounds, rng=0, **kw)
    _, _, zero = pybo_amd.solve_bayesopt(loop_objective, bounds, rng=0, batch_fantasies=0, **kw)
    np.testing.assert_array_equal(plain.x, zero.x)                    # the default is the believer's loop, untouched
    assert not np.array_equal(plain.x, info.x)
