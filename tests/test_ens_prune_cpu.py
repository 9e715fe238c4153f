"""Selection-only ensemble sweeps, the parts that need no GPU: (a) the one new step of the argument --
bounds that dominate member by member still dominate after the member-order sum and the division by n, bit for bit, and
a NaN member gives a NaN sum; (b) the oracle's own survivor count for every shared case, so that the device test's
"path == pruned" cannot fail merely because the inputs bound loosely."""
import numpy as np
import pytest

from oracle import gp_ref
import ens_prune_cases as cases


def _special(rng, shape):
    """Non-negative doubles over the whole range with 0, denormals and +inf mixed in."""
    v = np.exp(rng.uniform(-740.0, 700.0, size=shape))
    pick = rng.randint(0, 12, size=shape)
    v[pick == 0] = 0.0
    v[pick == 1] = 5e-324 * rng.randint(1, 1000, size=shape)[pick == 1]
    v[pick == 2] = np.inf
    return v


@pytest.mark.parametrize('n', [1, 2, 3, 4, 10])
def test_the_member_order_mean_of_dominating_bounds_dominates(n):
    rng = np.random.RandomState(n)
    m = 200000
    v = _special(rng, (n, m))
    # ub >= v elementwise: equal, one ulp above, a relative margin, an absolute margin, +inf
    how = rng.randint(0, 5, size=(n, m))
    with np.errstate(over='ignore', invalid='ignore'):
        ub = np.select([how == 0, how == 1, how == 2, how == 3], [v, np.nextafter(v, np.inf), v * (1.0 + 1e-6), v + 1e-9], np.inf)
    nan = rng.rand(n, m) < 0.01
    v[nan] = np.nan
    ub[nan] = np.nan
    assert np.all((ub >= v) | nan)
    with np.errstate(over='ignore', invalid='ignore'):
        mv, mub = cases.ens_mean(list(v)), cases.ens_mean(list(ub))
    any_nan = nan.any(axis=0)
    assert np.array_equal(np.isnan(mub), any_nan) and np.array_equal(np.isnan(mv), any_nan)
    assert np.all(mub[~any_nan] >= mv[~any_nan])


_ORACLE = {}


def _oracle(name):
    """Per case, once: the members' means and variances at every candidate (float64 oracle), their exact EI and the bound
    EI(mu_m + 1e-9, sqrt(rho_m)) (1e-9 stands for the device's margin delta_m = 8 (Np + 16) 2^-53 (rho S + |bias|), which the
    device reports as 2.6e-9 .. 9.9e-9 at N = 1153: either is far below the gap between tau and the bounds of what is left out)."""
    if name not in _ORACLE:
        p = cases.problem(name)
        val, ub = [], []
        for sn2, rho, ell, bias in p['hypers']:
            r = gp_ref.make_gp(sn2, rho, ell, bias, p['kernel'])
            r.add_data(p['X'], p['y'])
            mu, s2 = r.predict(p['Z'])
            val.append(cases.ei(mu, np.sqrt(s2), p['target']))
            ub.append(cases.ei(mu + 1e-9, np.sqrt(rho), p['target']))
        _ORACLE[name] = (p, cases.ens_mean(val), cases.ens_mean(ub))
    return _ORACLE[name]


@pytest.mark.parametrize('k', cases.KS)
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_the_oracle_s_survivors_stay_inside_half_the_cap(name, k):
    p, val, ub = _oracle(name)
    assert np.all(ub >= val)
    seeds, tau, surv = cases.survivors(ub, lambda i: val[i], k)
    print('%s k=%d: tau %.4g, survivors %d of %d, cap %d' % (name, k, tau, len(surv), len(val), cases.cap_of(len(val))))
    assert tau >= 1e-280
    assert len(surv) <= cases.cap_of(len(val)) // 2
    # and the selection loses nothing: the k best of everything lie among the seeds and the survivors
    best = gp_ref.topk_desc(val, k)
    assert set(best.tolist()) <= set(seeds.tolist()) | set(surv.tolist())
