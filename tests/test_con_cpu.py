"""Constrained optimisation, the parts that need no GPU: (a) the oracle's own survivor count for every
shared case of con_cases.py, so that the device test's "path == pruned" cannot fail merely because the objective's EI bound is loose
against the PRODUCT; (b) models.Constrained over oracle members: column routing, values against con_ref.py, gradients against central
differences; (c) the incumbent rule of policies.CEI and recommenders.best_feasible, both branches each; (d) a solve_bayesopt run."""
import numpy as np
import pytest

from oracle import gp_ref
import con_cases as cases
import con_ref
import ens_prune_cases
from pybo_amd import models, policies, recommenders, solve_bayesopt

_ORACLE = {}


def _oracle(name):
    """Per case, once: the oracle's cEI and EI at every candidate and the objective's bound EI(mu + 1e-9, sqrt(rho)) (1e-9 stands
    for the device's margin delta, as in test_ens_prune_cpu.py)."""
    if name not in _ORACLE:
        p = cases.problem(name)
        obj, cons = con_ref.models(p)
        val = con_ref.values(obj, cons, p['thr'], 'ei', p['target'], p['Z'])[0]
        mu, s2 = obj.predict(p['Z'])
        ub = ens_prune_cases.ei(mu + 1e-9, np.sqrt(obj.rho), p['target'])
        _ORACLE[name] = (p, val, ens_prune_cases.ei(mu, np.sqrt(s2), p['target']), ub)
    return _ORACLE[name]


@pytest.mark.parametrize('k', cases.KS)
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_the_oracle_s_survivors_stay_inside_half_the_cap(name, k):
    p, val, ei, ub = _oracle(name)
    assert np.all(ub >= ei) and np.all(ei >= val) and np.all(ub >= val)
    seeds, tau, surv = ens_prune_cases.survivors(ub, lambda i: val[i], k)
    cap = cases.cap_of(len(val))
    print('%s k=%d: tau %.4g, survivors %d of %d, cap %d' % (name, k, tau, len(surv), len(val), cap))
    assert cap == max(4096, len(val) // 4)
    assert tau >= 1e-280
    assert len(surv) <= cap // 2
    # the selection loses nothing: the k best of everything lie among the seeds and the survivors
    best = gp_ref.topk_desc(val, k)
    assert set(best.tolist()) <= set(seeds.tolist()) | set(surv.tolist())
    # and the constraints matter: the constrained top-k is not the objective's
    assert not np.array_equal(best, gp_ref.topk_desc(ei, k))


# ---- (b) models.Constrained over oracle members ----------------------------------------------------------------------------------
def _small(J=2, n=40, d=3, seed=3):
    p = cases.build(n, d, 'se', seed, J, m=64)
    obj = gp_ref.make_gp(*p['hypers'][0], 'se')
    cons = [gp_ref.make_gp(*h, 'se') for h in p['hypers'][1:]]
    return p, models.Constrained(obj, cons, thresholds=p['thr'])


def test_add_data_routes_the_columns():
    p, model = _small()
    Y = np.column_stack([p['y'], p['C']])
    model.add_data(p['X'][:30], Y[:30])
    model.add_data(p['X'][30], Y[30])                      # one point, (1 + J,): what objective(x) returns in the loop
    model.add_data(p['X'][31:], Y[31:])
    assert model.ndata == 40
    assert np.array_equal(model.objective.Y, p['y'])
    for j, c in enumerate(model.constraints):
        assert np.array_equal(c.Y, p['C'][:, j]) and np.array_equal(c.X, p['X'])
    with pytest.raises(ValueError):
        model.add_data(p['X'][:2], Y[:2, :2])
    other = model.copy()
    other.add_data(p['X'][0], Y[0])
    assert other.ndata == 41 and model.ndata == 40         # a copy's data are its own
    mu, s2 = model.predict(p['Z'])
    want = model.objective.predict(p['Z'])
    assert np.array_equal(mu, want[0]) and np.array_equal(s2, want[1]) and np.array_equal(model.predict_mean(p['Z']), want[0])
    with pytest.raises(ValueError):
        models.Constrained(model.objective, [])
    assert np.array_equal(models.Constrained(model.objective, model.constraints).thresholds, [0.0, 0.0])


@pytest.mark.parametrize('J', [1, 2, 3])
def test_values_and_gradients(J):
    p, model = _small(J)
    model.add_data(p['X'], np.column_stack([p['y'], p['C']]))
    obj, cons = con_ref.models(p)
    Z = p['Z']
    v, w, _, _ = con_ref.values(obj, cons, p['thr'], 'ei', p['target'], Z)
    assert np.array_equal(model.get_constrained(p['target'], Z), v)
    assert np.array_equal(model.feasibility(Z), w) and np.array_equal(model.get_constrained(None, Z), w)
    assert np.all((w >= 0.0) & (w <= 1.0)) and np.all(v <= obj.get_improvement(p['target'], Z)) and w.min() < 0.5 < w.max()
    for target in (p['target'], None):
        f, g = model.get_constrained(target, Z[:8], grad=True)
        fr, gr = con_ref.value_grad(obj, cons, p['thr'], target, Z[:8])
        np.testing.assert_allclose(f, fr, rtol=1e-13, atol=0)
        np.testing.assert_allclose(g, gr, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(f, model.get_constrained(target, Z[:8]), rtol=1e-13, atol=0)
        h = 1e-6
        for j in range(Z.shape[1]):
            e = np.zeros(Z.shape[1])
            e[j] = h
            num = (model.get_constrained(target, Z[:8] + e) - model.get_constrained(target, Z[:8] - e)) / (2 * h)
            np.testing.assert_allclose(g[:, j], num, rtol=2e-6, atol=1e-9 * np.abs(f).max())
    f, g = model.feasibility(Z[:4], grad=True)
    assert np.array_equal(f, model.get_constrained(None, Z[:4], grad=True)[0]) and g.shape == (4, Z.shape[1])


# ---- (c) the incumbent rules ---------------------------------------------------------------------------------------------------
def _fitted(thr_shift=0.0):
    p, model = _small()
    model.thresholds = model.thresholds + thr_shift
    model.add_data(p['X'], np.column_stack([p['y'], p['C']]))
    return p, model


def test_cei_takes_the_best_probably_feasible_observation_as_its_incumbent():
    p, model = _fitted()
    X, Z = p['X'], p['Z']
    pof = model.feasibility(X)
    ok = pof >= 0.5
    assert 0 < ok.sum() < len(X)
    mu = model.predict_mean(X)
    assert mu[ok].max() < mu.max()                         # the best observation of all is NOT feasible: the rule shows
    index = policies.CEI(model, None, X, xi=0.01)
    assert index.acq == ('cei', mu[ok].max() + 0.01)
    assert np.array_equal(index(Z), model.get_constrained(mu[ok].max() + 0.01, Z))
    f, g = index(Z[:3], grad=True)
    assert f.shape == (3,) and g.shape == (3, Z.shape[1])
    assert not hasattr(index, 'batch') and not hasattr(index, 'topk')      # (oracle members: no device sweep)
    # a stricter pmin moves the incumbent
    strict = policies.CEI(model, None, X, pmin=0.9)
    assert strict.acq[1] == mu[pof >= 0.9].max() <= index.acq[1]
    with pytest.raises(TypeError):
        policies.CEI(model.objective, None, X)


def test_cei_without_a_feasible_observation_is_the_probability_of_feasibility():
    p, model = _fitted(thr_shift=10.0)
    X, Z = p['X'], p['Z']
    assert model.feasibility(X).max() < 0.5
    index = policies.CEI(model, None, X)
    assert index.acq == ('cei', None)
    assert np.array_equal(index(Z), model.feasibility(Z))
    # pmin is the rule: a threshold nobody reaches says the same on a feasible problem
    p, model = _fitted()
    assert policies.CEI(model, None, p['X'], pmin=1.5).acq == ('cei', None)


def test_best_feasible():
    p, model = _fitted()
    X = p['X']
    pof, mu = model.feasibility(X), model.predict_mean(X)
    ok = pof >= 0.5
    want = X[np.flatnonzero(ok)[np.argmax(mu[ok])]]
    assert np.array_equal(recommenders.best_feasible(model, None, X), want)
    assert not np.array_equal(want, recommenders.best_incumbent(model, None, X))
    # nothing qualifies: the most feasible observation
    assert np.array_equal(recommenders.best_feasible(model, None, X, pmin=1.5), X[np.argmax(pof)])
    p, model = _fitted(thr_shift=10.0)
    assert np.array_equal(recommenders.best_feasible(model, None, p['X']), p['X'][np.argmax(model.feasibility(p['X']))])


# ---- (d) the loop ------------------------------------------------------------------------------------------------------------
def run_loop(make, capsys=None):
    """12 evaluations of f = -(x - 0.3)^2 subject to x0 - 0.5 >= 0 in 2-d (shared with test_gpu_constrained.py)."""
    bounds = [[0.0, 1.0], [0.0, 1.0]]
    model = models.Constrained(make(1e-4, 1.0, [0.3, 0.3], -0.2), [make(1e-4, 1.0, [0.4, 0.4], 0.0)], thresholds=[0.0])

    def objective(x):
        x = np.ravel(x)
        return float(-np.sum((x - 0.3) ** 2)), float(x[0] - 0.5)

    xbest, model, info = solve_bayesopt(objective, bounds, model=model, niter=12, policy='cei', recommender='feasible',
                                        solver=('lbfgs', {'ngrid': 400, 'nbest': 3}), verbose=True, rng=0)
    assert info.y.shape == (len(info.x), 2) and info.x.shape == (len(info.x), 2) and len(info.xbest) == 12
    assert np.array_equal(info.y[:, 1], info.x[:, 0] - 0.5)
    assert model.feasibility(xbest[None])[0] >= 0.5
    assert any(np.array_equal(xbest, x) for x in info.x)
    return xbest, model, info


def test_solve_bayesopt_with_cei_and_the_feasible_recommender(capsys):
    xbest, model, info = run_loop(lambda sn2, rho, ell, bias: gp_ref.make_gp(sn2, rho, ell, bias))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('i=')]
    assert len(lines) == 12 and all(', y=' in ln and 'xbest=[' in ln for ln in lines)
    # the progress line shows the objective column
    assert 'y={: .3f}'.format(info.y[-1, 0]) in lines[-1]
