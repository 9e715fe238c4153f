"""Batch proposals on the host (no GPU): the generic path of pybo_amd.propose_batch over the oracle's GPRef against the
from-scratch greedy of tests/batch_ref.py, what the policies hand to it, and solve_bayesopt(..., nbatch=)."""
import numpy as np
import pytest

import batch_ref
from oracle import gp_ref
from helpers import loop_objective

import pybo_amd
from pybo_amd import policies

BOUNDS2 = np.array([[0.0, 1.0], [0.0, 1.0]])


def _frozen(kind, param):
    """A policy whose index carries the case's own parameter (the policies derive theirs from the model)."""
    def policy(model, bounds, X):
        def index(X, grad=False):
            raise AssertionError('the batch path scores through the model protocol')
        index.acq = (kind, param)
        return index
    return policy


@pytest.mark.parametrize('tag', ['se_300_3_ei', 'matern1_130_5_pi'])
def test_the_generic_host_path_equals_the_from_scratch_greedy(tag):
    prob, ref = batch_ref.case(tag)
    assert ref['margin'].min() >= batch_ref.MIN_MARGIN
    gp = gp_ref.make_gp(prob['sn2'], prob['rho'], prob['ell'], prob['bias'], prob['kernel'])
    gp.add_data(prob['X'], prob['y'])
    d = prob['X'].shape[1]
    Xq, vals, idx = pybo_amd.propose_batch(gp, [[0.0, 1.0]] * d, prob['X'], prob['nb'], policy=_frozen(prob['kind'], prob['param']),
                                           xgrid=prob['Z'])
    np.testing.assert_array_equal(idx, ref['idx'])
    np.testing.assert_array_equal(Xq, prob['Z'][ref['idx']])
    np.testing.assert_allclose(vals, ref['val'], rtol=1e-9)           # the same arithmetic on a model grown by add_data
    assert gp.ndata == len(prob['X'])                                 # the caller's model is left alone


def test_the_index_carries_the_policys_own_parameter():
    prob, _ = batch_ref.case('se_300_3_ei')
    gp = gp_ref.make_gp(prob['sn2'], prob['rho'], prob['ell'], prob['bias'], prob['kernel'])
    gp.add_data(prob['X'], prob['y'])
    X = prob['X']
    top = gp.predict(X)[0].max()
    assert policies.EI(gp, None, X, xi=0.01).acq == ('ei', top + 0.01)
    assert policies.PI(gp, None, X).acq == ('pi', top + 0.05)
    kind, beta = policies.UCB(gp, None, X, delta=0.1, xi=0.2).acq
    n = len(X)
    assert kind == 'ucb' and beta == 0.2 * 2 * np.log(np.pi ** 2 / 3 / 0.1) + 0.2 * (4 + n) * np.log(n + 1)
    assert not hasattr(policies.EI(gp, None, X), 'batch')             # a host model has no device path
    assert not hasattr(policies.Thompson(gp, None, X, n=20, rng=0), 'acq')
    # ... and propose_batch scores with exactly that parameter
    _, vals, idx = pybo_amd.propose_batch(gp, [[0.0, 1.0]] * 3, X, 1, policy=('ei', {'xi': 0.01}), xgrid=prob['Z'])
    ei = gp.get_improvement(top + 0.01, prob['Z'])
    assert idx[0] == int(np.argmax(ei)) and vals[0] == ei[idx[0]]


def test_thompson_gives_independent_draws():
    prob, _ = batch_ref.case('se_300_3_ei')
    gp = gp_ref.make_gp(prob['sn2'], prob['rho'], prob['ell'], prob['bias'], prob['kernel'])
    gp.add_data(prob['X'], prob['y'])
    Z = prob['Z'][:500]
    Xq, vals, idx = pybo_amd.propose_batch(gp, [[0.0, 1.0]] * 3, prob['X'], 4, policy=('thompson', {'n': 50}), xgrid=Z, rng=3)
    rng = np.random.RandomState(3)
    want = [int(np.argmax(gp.sample_f(50, rng).get(Z))) for _ in range(4)]
    assert list(idx) == want and Xq.shape == (4, 3)


def _loop_model():
    gp = gp_ref.make_gp(1e-4, 1.0, [0.3, 0.35], 0.0)
    X0 = np.random.RandomState(2).rand(6, 2)
    gp.add_data(X0, [loop_objective(x) for x in X0])
    return gp


GRID = np.random.RandomState(7).rand(400, 2)


def test_solve_bayesopt_in_batches_counts_evaluations_and_resumes(tmp_path):
    calls = []

    def objective(x):
        assert np.shape(x) == (2,)                     # one call per row
        calls.append(np.array(x))
        return loop_objective(x)

    kw = dict(model=_loop_model(), policy='ei', recommender='incumbent', nbatch=3, batch_grid=GRID, rng=0)
    xbest, model, info = pybo_amd.solve_bayesopt(objective, BOUNDS2, niter=10, **kw)
    assert len(info.x) == len(info.y) == 11 and len(info.xbest) == 10          # the box centre + 10 evaluations
    assert len(calls) == 11 and model.ndata == 6 + 11
    np.testing.assert_array_equal(np.array(calls), info.x)
    # batches of 3, 3, 3 and a truncated one: one recommendation per batch, repeated per point
    xb = info.xbest
    for lo, hi in ((0, 3), (3, 6), (6, 9), (9, 10)):
        assert np.all(xb[lo:hi] == xb[lo])
    grid_rows = {tuple(r) for r in GRID}
    assert all(tuple(x) in grid_rows for x in info.x[1:])
    assert len({tuple(x) for x in info.x}) == 11                               # believer conditioning: no point twice

    # interrupted after two batches, resumed from the checkpoint: the same trace
    log = str(tmp_path / 'run.pkl')
    n0 = len(calls)
    _, _, part = pybo_amd.solve_bayesopt(objective, BOUNDS2, niter=6, log=log, **kw)
    assert len(part.xbest) == 6 and len(calls) - n0 == 7
    _, model2, full = pybo_amd.solve_bayesopt(objective, BOUNDS2, niter=10, log=log, **kw)
    assert len(calls) - n0 == 11                                               # only the four missing evaluations
    for a, b in zip(full, info):
        np.testing.assert_array_equal(a, b)
    assert model2.ndata == model.ndata


def test_nbatch_one_is_the_plain_loop():
    kw = dict(model=_loop_model(), niter=5, policy='ei', recommender='incumbent', solver=('lbfgs', {'xgrid': GRID, 'nbest': 3}),
              rng=0)
    _, _, a = pybo_amd.solve_bayesopt(loop_objective, BOUNDS2, **kw)
    _, _, b = pybo_amd.solve_bayesopt(loop_objective, BOUNDS2, nbatch=1, **kw)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_batches_do_not_combine_with_spmd():
    with pytest.raises(ValueError, match='spmd'):
        pybo_amd.solve_bayesopt(loop_objective, BOUNDS2, model=_loop_model(), niter=4, nbatch=2, spmd=True)
    with pytest.raises(ValueError):
        pybo_amd.solve_bayesopt(loop_objective, BOUNDS2, model=_loop_model(), niter=4, nbatch=0)
