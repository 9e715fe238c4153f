"""Two-objective optimisation, the parts that need no GPU.  (a) The yardstick: the reference closed form of
ehvi_ref.py against (i) the per-sample identity HV(P + {y}) - HV(P) = sum over the strips, to 1e-12, and (ii) Monte Carlo with a fixed
seed and 2e5 draws, within 5 standard errors -- both pass without the feature.  Everything after needs it: (b) pybo_amd/pareto.py against
the reference; (c) models.MultiObjective over oracle and stub members: column routing, values, the gradient against central differences;
(d) policies.EHVI and recommenders.best_pareto: the default reference point, ties; (e) a 12-iteration solve_bayesopt run."""
import numpy as np
import pytest

from oracle import gp_ref
import ehvi_cases as cases
import ehvi_ref
from helpers import SmootherModel

# (front size, seed, moments of the four MC cases: mu1, s1, mu2, s2)
MC_CASES = [(0, 1, (0.1, 0.5, -0.2, 0.8)), (1, 2, (0.0, 1.0, 0.0, 1.0)), (7, 3, (0.3, 0.4, -0.1, 0.6)), (64, 4, (-0.5, 1.5, 0.4, 0.2))]


# ---- (a) the yardstick (passes without the feature) ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 2, 7, 64])
def test_reference_strips_add_up_to_the_hypervolume_difference_per_sample(n):
    rng = np.random.RandomState(10 + n)
    P, ref = cases.raw_front(n, seed=n) if n else (np.empty((0, 2)), np.array([-1.5, -1.5]))
    a, b = ehvi_ref.strips(P, ref)
    assert len(b) == n + 1 and len(a) == n + 2
    Y = rng.uniform(-2.5, 2.0, size=(300, 2))
    Y[:20] = P[rng.randint(0, len(P), size=20)] if n else Y[:20]          # samples on front points, duplicates and edges themselves
    base = ehvi_ref.hypervolume(P, ref)
    for y, got in zip(Y, ehvi_ref.hvi_strips(Y, a, b)):
        want = ehvi_ref.hypervolume(np.vstack([P, y[None]]), ref) - base
        assert abs(got - want) <= 1e-12, (y, got, want)
    assert np.all(ehvi_ref.hvi_strips(Y[(Y[:, 0] <= ref[0]) | (Y[:, 1] <= ref[1])], a, b) == 0.0)


@pytest.mark.parametrize('n,seed,mom', MC_CASES)
def test_reference_closed_form_against_monte_carlo(n, seed, mom):
    P, ref = cases.raw_front(n, seed=seed) if n else (np.empty((0, 2)), np.array([-1.5, -1.5]))
    a, b = ehvi_ref.strips(P, ref)
    mu1, s1, mu2, s2 = mom
    rng = np.random.RandomState(100 + seed)
    Y = np.column_stack([mu1 + s1 * rng.randn(200000), mu2 + s2 * rng.randn(200000)])
    h = ehvi_ref.hvi_strips(Y, a, b)
    want = ehvi_ref.ehvi(mu1, s1 * s1, mu2, s2 * s2, a, b)[0]
    se = h.std(ddof=1) / np.sqrt(len(h))
    print('n=%d: closed form %.6g, MC %.6g, %.2f standard errors' % (n, want, h.mean(), (h.mean() - want) / se))
    assert want > 0 and abs(h.mean() - want) <= 5.0 * se


# ---- (b) pybo_amd/pareto.py ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 7, 64])
def test_pareto_module_against_the_reference(n):
    from pybo_amd import pareto
    P, ref = cases.raw_front(n, seed=n) if n else (np.empty((0, 2)), np.array([-1.5, -1.5]))
    a, b = pareto.strips(P, ref)
    ra, rb = ehvi_ref.strips(P, ref)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    assert abs(pareto.hypervolume(P, ref) - ehvi_ref.hypervolume(P, ref)) <= 1e-12
    mask = pareto.pareto_mask(P)
    assert mask.shape == (len(P),)
    above = (P[:, 0] > ref[0]) & (P[:, 1] > ref[1])
    F = ehvi_ref.front(P, ref)
    if n:
        assert np.array_equal(np.unique(P[mask & above], axis=0), F) and len(P[mask & above]) == len(F)      # one copy of duplicates
    c = pareto.hv_contributions(P, ref)
    for i in range(0, len(P), max(1, len(P) // 12)):
        want = ehvi_ref.hypervolume(P, ref) - ehvi_ref.hypervolume(np.delete(P, i, axis=0), ref)
        assert abs(c[i] - want) <= 1e-12
    mom = cases.synthetic_moments(500, seed=n)[:, 2:]
    got = pareto.ehvi_from_moments(*mom, a, b)
    want, S = ehvi_ref.ehvi(*mom, a, b), ehvi_ref.magnitude(*mom, a, b)
    assert np.all(np.abs(got - want) <= 1e-12 * S + ehvi_ref.TINY)
    assert np.all(got >= 0.0)


def test_pareto_nan_and_empty_front():
    from pybo_amd import pareto
    a, b = pareto.strips(np.empty((0, 2)), [0.0, 1.0])
    assert np.array_equal(a, [0.0, np.inf]) and np.array_equal(b, [1.0])
    v = pareto.ehvi_from_moments([0.5, np.nan, 0.5], [1.0, 1.0, 1.0], [0.2, 0.2, np.nan], [0.5, 0.5, 0.5], a, b)
    assert np.isnan(v[1]) and np.isnan(v[2])
    assert v[0] == max(ehvi_ref.ei(0.5, 1.0, 0.0), 0.0) * ehvi_ref.ei(0.2, np.sqrt(0.5), 1.0)
    assert np.array_equal(pareto.default_ref([[1.0, 5.0], [3.0, 5.0]]), [0.8, 4.9])      # span 0 counts as 1


# ---- (c) models.MultiObjective ---------------------------------------------------------------------------------------------------
def _small(n=40, d=3, seed=3):
    from pybo_amd import models
    p = cases.build(n, d, 'se', seed, m=64)
    model = models.MultiObjective(*[gp_ref.make_gp(*h, k) for h, k in zip(p['hypers'], p['kernels'])])
    return p, model


def test_add_data_routes_the_columns():
    from pybo_amd import models
    p, model = _small()
    model.add_data(p['X'][:30], p['Y'][:30])
    model.add_data(p['X'][30], p['Y'][30])                 # one point, (2,): what objective(x) returns in the loop
    model.add_data(p['X'][31:], p['Y'][31:])
    assert model.ndata == 40
    for j, m in enumerate(model.objectives):
        assert np.array_equal(m.Y, p['Y'][:, j]) and np.array_equal(m.X, p['X'])
    with pytest.raises(ValueError):
        model.add_data(p['X'][:2], np.ones((2, 3)))
    other = model.copy()
    other.add_data(p['X'][0], p['Y'][0])
    assert other.ndata == 41 and model.ndata == 40
    F = model.predict_mean(p['Z'])
    assert F.shape == (64, 2)
    for j, m in enumerate(model.objectives):
        assert np.array_equal(F[:, j], m.predict(p['Z'])[0])
    stub = models.MultiObjective(SmootherModel(), SmootherModel(ell=0.4))
    stub.add_data(p['X'], p['Y'])
    assert stub.predict_mean(p['Z']).shape == (64, 2) and stub.anticipate(p['Z'][0]) is False
    front = stub.pareto_set(p['X'])
    assert 1 <= len(front) <= 40 and all(any(np.array_equal(f, x) for x in p['X']) for f in front)


def test_get_ehvi_values_and_gradient():
    from pybo_amd import pareto
    p, model = _small()
    model.add_data(p['X'], p['Y'])
    ms = ehvi_ref.models(p)
    front = model.predict_mean(p['X'])
    ref = pareto.default_ref(front)
    a, b = ehvi_ref.strips(front, ref)
    assert len(b) - 1 >= 3                                  # a front worth the name
    Z = p['Z']
    want, _, moms = ehvi_ref.values(ms, a, b, Z)
    S = ehvi_ref.magnitude(*moms, a, b)
    got = model.get_ehvi(front, ref, Z)
    assert np.all(np.abs(got - want) <= 1e-12 * S + ehvi_ref.TINY) and got.max() > 0
    f, g = model.get_ehvi(front, ref, Z[:8], grad=True)
    assert np.array_equal(f, got[:8]) and g.shape == (8, Z.shape[1])
    h = 1e-6
    for j in range(Z.shape[1]):
        e = np.zeros(Z.shape[1])
        e[j] = h
        num = (model.get_ehvi(front, ref, Z[:8] + e) - model.get_ehvi(front, ref, Z[:8] - e)) / (2 * h)
        np.testing.assert_allclose(g[:, j], num, rtol=2e-6, atol=1e-9 * np.abs(f).max())
    # an empty front: the product of the two EIs over the reference point
    f0 = model.get_ehvi(np.empty((0, 2)), ref, Z)
    assert np.allclose(f0, ms[0].get_improvement(ref[0], Z) * ms[1].get_improvement(ref[1], Z), rtol=1e-12, atol=0)


# ---- (d) the policy and the recommender ------------------------------------------------------------------------------------------
def test_ehvi_policy_default_reference_point_and_index():
    from pybo_amd import pareto, policies
    p, model = _small()
    model.add_data(p['X'], p['Y'])
    F = model.predict_mean(p['X'])
    index = policies.EHVI(model, None, p['X'])
    kind, (front, ref) = index.acq
    assert kind == 'ehvi' and np.array_equal(front, F)
    span = F.max(0) - F.min(0)
    assert np.array_equal(ref, F.min(0) - 0.1 * span) and np.all(ref < F.min(0))
    assert np.array_equal(index(p['Z']), model.get_ehvi(F, ref, p['Z']))
    f, g = index(p['Z'][:3], grad=True)
    assert f.shape == (3,) and g.shape == (3, p['Z'].shape[1])
    assert not hasattr(index, 'batch') and not hasattr(index, 'topk')      # (oracle members: no device sweep)
    mine = policies.EHVI(model, None, p['X'], ref=[-3.0, -2.0])
    assert np.array_equal(mine.acq[1][1], [-3.0, -2.0]) and np.all(mine(p['Z']) >= index(p['Z']))      # a lower reference point: more to gain
    with pytest.raises(TypeError):
        policies.EHVI(model.objectives[0], None, p['X'])
    # one observation: both spans are 0 and count as 1
    one = _small()[1]
    one.add_data(p['X'][:1], p['Y'][:1])
    F1 = one.predict_mean(p['X'][:1])
    assert np.array_equal(policies.EHVI(one, None, p['X'][:1]).acq[1][1], F1[0] - 0.1)
    assert pareto.default_ref(F1).shape == (2,)


class _MeansModel(object):
    """predict_mean returns the rows of a table: the recommender's rules on chosen numbers."""
    def __init__(self, F):
        self.F = np.asarray(F, dtype=float)

    def predict_mean(self, X):
        return self.F[:len(X)]

    def pareto_set(self, X):
        from pybo_amd import pareto
        return np.asarray(X)[pareto.pareto_mask(self.F[:len(X)])]


def test_best_pareto_and_its_ties():
    from pybo_amd import pareto, recommenders
    X = np.arange(10.0).reshape(5, 2)
    F = [[1.0, 4.0], [2.0, 3.0], [4.0, 1.0], [1.5, 1.5], [0.5, 0.5]]
    ref = pareto.default_ref(F)
    c = pareto.hv_contributions(F, ref)
    assert c[3] == 0.0 and c[4] == 0.0 and np.all(c[:3] > 0)
    assert np.array_equal(recommenders.best_pareto(_MeansModel(F), None, X), X[int(np.argmax(c))])
    # a symmetric front: the two ends contribute the same area, the lower index wins
    Fs = [[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]]
    cs = pareto.hv_contributions(Fs, [0.0, 0.0])
    assert cs[0] == cs[2] == 1.0 and cs[1] == 1.0
    assert np.array_equal(recommenders.best_pareto(_MeansModel(Fs), None, X[:3], ref=[0.0, 0.0]), X[0])
    # duplicates contribute nothing; a single observation is its own answer
    assert np.array_equal(pareto.hv_contributions([[1.0, 1.0], [1.0, 1.0]], [0.0, 0.0]), [0.0, 0.0])
    assert np.array_equal(recommenders.best_pareto(_MeansModel(F), None, X[:1]), X[0])
    p, model = _small()
    model.add_data(p['X'], p['Y'])
    xb = recommenders.best_pareto(model, None, p['X'])
    Fm = model.predict_mean(p['X'])
    assert np.array_equal(xb, p['X'][int(np.argmax(pareto.hv_contributions(Fm, pareto.default_ref(Fm))))])
    assert any(np.array_equal(xb, x) for x in model.pareto_set(p['X']))


# ---- (e) the loop ------------------------------------------------------------------------------------------------------------
def run_loop(make):
    """12 evaluations of the two-objective toy f1 = -|x - (0.2, 0.2)|^2, f2 = -|x - (0.8, 0.8)|^2 in 2-d (shared with test_gpu_ehvi.py)."""
    from pybo_amd import models, pareto, solve_bayesopt
    bounds = [[0.0, 1.0], [0.0, 1.0]]
    model = models.MultiObjective(make(1e-4, 1.0, [0.4, 0.4], -0.3), make(1e-4, 1.0, [0.4, 0.4], -0.3))

    def objective(x):
        x = np.ravel(x)
        return float(-np.sum((x - 0.2) ** 2)), float(-np.sum((x - 0.8) ** 2))

    rng = np.random.RandomState(0)
    X0 = rng.rand(4, 2)
    model.add_data(X0, [objective(x) for x in X0])
    ref = np.array([-1.5, -1.5])
    hv0 = pareto.hypervolume(model.predict_mean(X0), ref)
    xbest, model, info = solve_bayesopt(objective, bounds, model=model, niter=12, policy='ehvi', recommender='pareto',
                                        solver=('lbfgs', {'ngrid': 400, 'nbest': 3}), verbose=True, rng=0)
    assert info.y.shape == (len(info.x), 2) and info.x.shape == (len(info.x), 2) and len(info.xbest) == 12
    X = np.vstack([X0, info.x])
    hv1 = pareto.hypervolume(model.predict_mean(X), ref)
    print('hypervolume of the posterior means: %.4f -> %.4f' % (hv0, hv1))
    assert hv1 >= hv0
    assert any(np.array_equal(xbest, x) for x in info.x)
    return xbest, model, info


def test_solve_bayesopt_with_ehvi_and_the_pareto_recommender(capsys):
    xbest, model, info = run_loop(lambda sn2, rho, ell, bias: gp_ref.make_gp(sn2, rho, ell, bias))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('i=')]
    assert len(lines) == 12 and all(', y=' in ln and 'xbest=[' in ln for ln in lines)
    assert 'y={: .3f}'.format(info.y[-1, 0]) in lines[-1]      # the progress line shows the first objective
