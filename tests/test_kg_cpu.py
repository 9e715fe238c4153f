"""The knowledge gradient without a GPU: the ABI, the numpy closure of pybo_amd/kg.py against the 50-digit truth within the bound
kg_math.h derives, the analytic gradient against central differences, the teeth of the oracle (two mutations it must see), and
the policy on stub models (support selection, refusals, what the index carries, the registry)."""
import os
import re

import numpy as np
import pytest

import kg_ref
from helpers import synth_problem

from pybo_amd import _lib, inits, kg, policies
from pybo_amd.bayesopt import get_component

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS2 = np.array([[0.0, 1.0], [0.0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_the_abi_knows_kg():
    hdr = open(os.path.join(ROOT, 'include', 'gpx.h')).read()
    assert re.search(r'\bGPX_ACQ_KG\s*=\s*32\b', hdr) and re.search(r'\bint\s+gpx_kg_grad\s*\(', hdr)
    assert _lib.ACQ_SUPPORT == {'kg': 32} and _lib.acq_id('kg') == 32 and _lib.acq_id('ei') == 0 and _lib.acq_id(32) == 32
    assert not set(_lib.ACQ.values()) & set(_lib.ACQ_SUPPORT.values())
    assert _lib.KG_MAX_SUPPORT == kg.KG_MAX_SUPPORT == 127
    res, args = _lib.SYMBOLS['gpx_kg_grad']
    assert len(args) == 7
    lib = _lib.load()
    assert lib.gpx_version() >= 680 and hasattr(lib, 'gpx_kg_grad')
    blob = open(_lib.LIB_PATH, 'rb').read()
    for text in (b'KG takes m * d finite support coordinates, m in [1, 127]', b'KG is not supported', b'k_kg_cross', b'k_acq_kg'):
        assert text in blob, text
    assert len(_lib.TIMER_NAMES) == 22                      # no new timer slot: KG accumulates in acq_topk
    p, n = _lib._acq_params(np.arange(6.0).reshape(3, 2))
    assert n == 6 and p.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]


# ---------------------------------------------------------------------------------------------------------------------
# the numpy closure against the truth
# ---------------------------------------------------------------------------------------------------------------------
def _sets():
    rng = np.random.RandomState(4)
    out = []
    for n in (1, 2, 3, 5, 64, 128):
        for scale in (1.0, 1e-3, 30.0):
            out.append((rng.randn(n), scale * rng.randn(n)))
        out.append((rng.randint(0, 4, n).astype(float), np.full(n, 0.25)))                 # equal slopes
        out.append((np.full(n, -0.75), rng.randn(n)))                                      # equal intercepts
        a, b = rng.randn(n), rng.randn(n)
        for j in range(1, n, 2):                                                           # duplicated lines
            a[j], b[j] = a[j - 1], b[j - 1]
        out.append((a, b))
        b = np.where(np.arange(n) < 3, -1.0 + 1.1 * np.arange(n), 0.3 * rng.randn(n))      # three concurrent lines
        a = np.where(np.arange(n) < 3, 0.5 - 0.7 * b, -50.0 - rng.rand(n))
        out.append((a, b))
        out.append((rng.randn(n), 1e-300 * (np.arange(n) % 7)))                            # slopes of 1e-300
        out.append((-45.0 * np.arange(n) - rng.rand(n), 1.0 + np.arange(n) + 0.1 * rng.rand(n)))     # |c| beyond 38
        out.append((-(7.5 + 0.25 * (np.arange(n) % 9)) * np.arange(n), 1.0 * np.arange(n)))           # around the switch at 8
    return out


def test_numpy_value_is_within_the_derived_bound_of_the_truth():
    worst = 0.0
    for a, b in _sets():
        got = float(kg.kg_value(a, b))
        want, bound = kg_ref.kg_truth(a, b), kg_ref.kg_bound(a, b)
        assert got >= 0.0 and abs(got - want) <= bound, (len(a), got, want, bound)
        if bound > 0:
            worst = max(worst, abs(got - want) / bound)
    print('worst error / bound: %.3g' % worst)
    # vectorised over leading axes, chunked
    rng = np.random.RandomState(1)
    A, B = rng.randn(7, 3, 9), rng.randn(7, 3, 9)
    v = kg.kg_value(A, B, chunk=4)
    assert v.shape == (7, 3) and v[2, 1] == kg.kg_value(A[2, 1], B[2, 1])


def test_h_is_tail_stable():
    import mpmath as mp
    for c in (0.0, -0.3, 1.0, -5.0, 7.999, 8.0, -8.5, 20.0, -37.0, 38.5):
        want = float(kg_ref._h(-abs(mp.mpf(c))))
        got = float(kg.kg_H(c))
        assert abs(got - want) <= kg_ref.KG_H_REL * want + 2.0 ** -1074, (c, got, want)
    assert kg.kg_H(39.0) == 0.0 and kg.kg_H(np.inf) == 0.0 and kg.kg_H(-np.inf) == 0.0
    # the naive sum phi(c) + c Phi(c) cancels c^2-fold out there and misses the bound the pieces above meet: the form matters
    from scipy.special import erfc
    c = -30.0
    naive = 0.39894228040143267794 * np.exp(-0.5 * c * c) + c * 0.5 * erfc(-c * 0.70710678118654752440)
    want = float(kg_ref._h(mp.mpf(c)))
    assert abs(naive - want) > kg_ref.KG_H_REL * want


def test_the_oracle_sees_a_dropped_line_0_and_a_padding_line():
    """Two mutations move the values: the tests built on the oracle can see those errors."""
    X, y, ell = synth_problem(60, 2, seed=2)
    model = kg_ref.make_model(X, y - 2.0, 'se', 0.5 * ell, 1.0, 1e-2, -2.0)             # all posterior means negative
    rng = np.random.RandomState(3)
    pool, Z = rng.rand(200, 2), rng.rand(40, 2)
    A = pool[np.argsort(model.predict(pool)[0])[:9]]              # a support set of LOW means: the candidate's own line carries the value
    alpha, beta = kg_ref.lines(model, A, Z)
    assert alpha.max() < 0.0
    base = kg.kg_value(alpha, beta)
    big = base >= 1e-3 * base.max()
    dropped = kg.kg_value(*kg_ref.drop_line0(alpha, beta))
    padded = kg.kg_value(*kg_ref.add_padding_line(alpha, beta))
    assert np.mean(np.abs(dropped - base)[big] > 1e-3 * base[big]) >= 0.5
    assert np.mean(np.abs(padded - base)[big] > 1e-3 * base[big]) >= 0.5          # (a line at 0 above every mean swallows the value)
    assert np.mean(np.abs(padded - base) > 1e-3 * base.max()) >= 0.1
    # and the truth agrees with the closure on both
    for a, b in (kg_ref.drop_line0(alpha[5], beta[5]), kg_ref.add_padding_line(alpha[5], beta[5])):
        assert abs(kg_ref.kg_truth(a, b) - float(kg.kg_value(a, b))) <= kg_ref.kg_bound(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the analytic gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['se', 'matern5', 'matern3'])
def test_analytic_gradient_against_central_differences(kernel):
    X, y, ell = synth_problem(40, 3, seed=6)
    model = kg_ref.make_model(X, y, kernel, 0.6 * ell, 1.2, 1e-2, 0.1)
    rng = np.random.RandomState(9)
    A, Z = rng.rand(7, 3), rng.rand(6, 3)
    f, g = kg_ref.kg_oracle_grad(model, A, Z)
    assert np.all(np.abs(f - kg.kg_value(*kg_ref.lines(model, A, Z))) <= 1e-14)
    hstep = 1e-5
    for t in range(3):
        Zp, Zm = Z.copy(), Z.copy()
        Zp[:, t] += hstep
        Zm[:, t] -= hstep
        fd = (kg.kg_value(*kg_ref.lines(model, A, Zp)) - kg.kg_value(*kg_ref.lines(model, A, Zm))) / (2 * hstep)
        # central differences: h^2 f''' / 6 truncation (|f'''| of order 1e2 here) + rounding eps |f| / h
        assert np.all(np.abs(fd - g[:, t]) <= 1e-6 * (1.0 + np.abs(g[:, t]))), (t, fd, g[:, t])
    assert np.abs(g).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# the policy on stubs
# ---------------------------------------------------------------------------------------------------------------------
class KnowStub(object):
    """mean = -(x - 0.3)^2 summed; get_knowledge logs its arguments."""

    def __init__(self, log=None):
        self.log = [] if log is None else log

    def copy(self):
        self.log.append('copy')
        return KnowStub(self.log)

    def predict(self, X, grad=False):
        X = np.array(X, ndmin=2, dtype=float)
        self.log.append('predict')
        return -((X - 0.3) ** 2).sum(1), np.ones(len(X))

    def get_knowledge(self, support, X, grad=False):
        self.log.append(('get_knowledge', np.array(support), bool(grad)))
        X = np.array(X, ndmin=2, dtype=float)
        v = X.sum(1)
        return (v, np.ones_like(X)) if grad else v


class NoKnow(object):
    def copy(self):
        return NoKnow()

    def predict(self, X, grad=False):
        X = np.array(X, ndmin=2, dtype=float)
        return X.sum(1), np.ones(len(X))


class Ensemble(KnowStub):
    def __init__(self, members):
        KnowStub.__init__(self)
        self.members = members

    def copy(self):
        return Ensemble(self.members)


def test_policy_default_support_is_the_best_posterior_means_in_order():
    Xobs = np.array([[0.3, 0.3], [0.9, 0.1]])
    m = KnowStub()
    index = policies.KG(m, BOUNDS2, Xobs, nsupport=5, ngrid=50, rng=7)
    assert m.log[0] == 'copy' and m.log.count('predict') == 1
    pool = np.vstack([inits.init_uniform(BOUNDS2, 50, 7), Xobs])
    mu = -((pool - 0.3) ** 2).sum(1)
    order = np.lexsort((np.arange(len(mu)), -mu))[:5]
    kind, support = index.acq
    assert kind == 'kg' and np.array_equal(support, pool[order]) and np.array_equal(support[0], Xobs[0])
    assert not hasattr(index, 'batch') and not hasattr(index, 'topk')
    Z = np.random.RandomState(0).rand(4, 2)
    assert np.array_equal(index(Z), Z.sum(1))
    v, g = index(Z, grad=True)
    assert g.shape == (4, 2)
    calls = [c for c in m.log if isinstance(c, tuple)]
    assert len(calls) == 2 and np.array_equal(calls[0][1], support) and calls[1][2] is True
    # ties: the lower index first
    flat = KnowStub()
    flat.predict = lambda X, grad=False: (np.zeros(len(np.atleast_2d(X))), np.ones(len(np.atleast_2d(X))))
    flat.copy = lambda: flat
    idx2 = policies.KG(flat, BOUNDS2, Xobs, nsupport=3, ngrid=10, rng=1)
    assert np.array_equal(idx2.acq[1], inits.init_uniform(BOUNDS2, 10, 1)[:3])


def test_policy_takes_a_given_support_and_refuses_what_it_must():
    Xobs = np.array([[0.3, 0.3]])
    S = np.random.RandomState(2).rand(127, 2)
    m = KnowStub()
    index = policies.KG(m, BOUNDS2, Xobs, support=S)
    assert np.array_equal(index.acq[1], S) and 'predict' not in m.log
    with pytest.raises(ValueError):
        policies.KG(KnowStub(), BOUNDS2, Xobs, nsupport=128)
    with pytest.raises(ValueError):
        policies.KG(KnowStub(), BOUNDS2, Xobs, nsupport=0)
    with pytest.raises(ValueError):
        policies.KG(KnowStub(), BOUNDS2, Xobs, support=np.zeros((128, 2)))
    with pytest.raises(TypeError, match='get_knowledge'):
        policies.KG(NoKnow(), BOUNDS2, Xobs)
    with pytest.raises(TypeError, match='get_knowledge'):
        policies.KG(Ensemble([KnowStub(), NoKnow()]), BOUNDS2, Xobs)
    ens = policies.KG(Ensemble([KnowStub(), KnowStub()]), BOUNDS2, Xobs, nsupport=2, ngrid=5, rng=0)
    assert ens.acq[0] == 'kg' and not hasattr(ens, 'topk') and not hasattr(ens, 'batch')
    from pybo_amd.models.sharded import ShardedGP
    assert not hasattr(ShardedGP, 'get_knowledge')


def test_registry_finds_kg_and_batch_refuses_it():
    import pybo_amd
    pol = get_component('kg', policies, 3)
    index = pol(KnowStub(), BOUNDS2, np.array([[0.3, 0.3]]))
    assert index.acq[0] == 'kg' and len(index.acq[1]) == 64
    pol2 = get_component(('kg', {'nsupport': 4, 'ngrid': 20}), policies, 3)
    assert len(pol2(KnowStub(), BOUNDS2, np.array([[0.3, 0.3]])).acq[1]) == 4
    assert 'KG' in policies.__all__
    with pytest.raises(ValueError, match='EI, PI or UCB'):
        pybo_amd.propose_batch(KnowStub(), BOUNDS2, np.array([[0.3, 0.3]]), 2, policy=('kg', {'nsupport': 3, 'ngrid': 10}), ngrid=10, rng=0)


def test_member_mean_sums_in_member_order_and_divides_once():
    outs = [np.array([0.1, 1e16]), np.array([0.2, -1e16]), np.array([0.3, 1.0])]
    want = ((outs[0] + outs[1]) + outs[2]) / 3
    assert np.array_equal(kg.member_mean(outs), want)
    from pybo_amd.models.mcmc import MCMC
    assert 'member_mean' in open(os.path.join(ROOT, 'pybo_amd', 'models', 'mcmc.py')).read() and hasattr(MCMC, 'get_knowledge')
