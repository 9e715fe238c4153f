"""Max-value entropy search without a GPU: the ABI, the teeth of tests/mes_ref.py's bound, the device's pieces of g emulated in numpy
against it, and the policy on the oracle's CPU model (Gumbel sampler, index, host gradient, the BO loop, the batch refusal)."""
import os
import re

import mpmath as mp
import numpy as np
import pytest
from scipy.special import log_ndtr

import mes_ref
from oracle import gp_ref
from helpers import loop_objective

import pybo_amd
from pybo_amd import _lib, inits, mes, policies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS2 = np.array([[0.0, 1.0], [0.0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_the_abi_knows_mes():
    hdr = open(os.path.join(ROOT, 'include', 'gpx.h')).read()
    assert re.search(r'\bGPX_ACQ_MES\s*=\s*16\b', hdr)
    assert _lib.ACQ['mes'] == 16 and sorted(_lib.ACQ.values()) == [0, 1, 2, 3, 16]
    lib = _lib.load()
    assert lib.gpx_version() >= 670
    blob = open(_lib.LIB_PATH, 'rb').read()
    for text in (b'MES takes 1 to 64 finite maximum samples', b'MES takes n_members * S maximum samples, S in [1, 64]',
                 b'MES is not supported', b'k_acq_mes'):
        assert text in blob, text


def test_one_helper_turns_a_parameter_into_the_pair():
    p, n = _lib._acq_params(None)
    assert n == 1 and p.tolist() == [0.0]
    p, n = _lib._acq_params(0.25)
    assert n == 1 and p.tolist() == [0.25]
    p, n = _lib._acq_params(np.float64(2.0))
    assert n == 1 and p.tolist() == [2.0]
    y = np.array([[1.0, 2.0], [3.0, 4.0]])
    p, n = _lib._acq_params(y)
    assert n == 4 and p.tolist() == [1.0, 2.0, 3.0, 4.0] and p.dtype == np.float64 and p.flags.c_contiguous
    assert _lib._acq_params(np.zeros(0))[1] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the bound has teeth, the pieces meet it
# ---------------------------------------------------------------------------------------------------------------------
def _check(cs, got):
    """check_mes with mu = 0, s2 = 1, y* = c, S = 1: gamma is the double c itself (its three roundings are exact here)."""
    cs = np.asarray(cs, dtype=float)
    return mes_ref.check_mes(np.zeros(len(cs)), np.ones(len(cs)), cs[:, None], got)


def test_the_naive_two_term_form_violates_the_bound():
    """Each term as accurate as a double allows, then subtracted: ~ gamma^2 u / g relative.  Every point from -1e3 on must violate."""
    cs = -np.array([1.0e3, 1.7e3, 4.0e3, 1.3e4, 1.0e5, 3.1e5, 1.0e6])
    bad, worst = _check(cs, mes_ref.naive_g_log(cs))
    assert bad.all() and worst > 1e3, (bad, worst)
    # ... and as one would first write it, it is not even finite there
    assert not np.isfinite(mes_ref.naive_g(cs)).any()


def _sweep():
    rng = np.random.RandomState(5)
    near = lambda c: c * (1 + np.arange(-8, 9) * 2.0 ** -52)        # noqa: E731
    return np.concatenate([
        -np.logspace(np.log10(8.0), 6, 120), -np.linspace(7.5, 8.5, 41), near(-8.0), -np.linspace(0.0, 8.0, 81)[1:],
        -np.logspace(-300, -1, 31), near(8.0), np.linspace(7.5, 8.5, 41), np.logspace(-300, -1, 31), np.linspace(0.0, 38.0, 153),
        np.linspace(37.0, 38.0, 21), rng.uniform(-40, 38, 60), [-1e6, 38.0]])


def test_the_pieces_of_g_meet_the_bound():
    cs = _sweep()
    assert cs.min() == -1e6 and cs.max() == 38.0
    bad, worst = _check(cs, mes.mes_g(cs))
    assert not bad.any(), (worst, cs[bad][:6])
    # the special points: +-0 -> log 2; 38.5: subnormal; +-inf; NaN
    sp = np.array([0.0, -0.0, 38.5, 38.6, 38.9, 39.0, 1e300, np.inf, -np.inf, np.nan, -1e50, -1e300])
    g = mes.mes_g(sp)
    bad, worst = _check(sp, g)
    assert not bad.any(), (worst, sp[bad], g[bad])
    assert g[0] == g[1] == np.log(2.0)
    assert 0.0 < g[2] < 2.0 ** -1022 and np.all(g[4:8] == 0.0) and not np.signbit(g[4:8]).any()
    assert g[8] == np.inf and np.isnan(g[9]) and np.isfinite(g[10:]).all()
    finite = g[np.isfinite(g)]
    assert np.all(finite >= 0.0) and not np.signbit(finite).any()


def test_the_bound_itself_stays_below_1e11_of_g():
    """S = 1, gamma in [-1e6, 38]: a derivation may not bless a cancelling implementation -- its bound is capped at 1e-11 g plus the
    subnormal term (conditioning alone is 1500 * 3 u = 5e-13 at the right end; the naive form errs by 1.5e-11 at -1e3)."""
    cs = _sweep()
    worst = 0.0
    for c in cs:
        t = mes_ref.mes_truth(0.0, 1.0, [c])
        b = mes_ref.mes_bound(0.0, 1.0, [c], t)
        assert b <= 1e-11 * float(t) + mes_ref.TINY, (c, b, float(t))
        worst = max(worst, (b - mes_ref.TINY) / float(t) if float(t) > 1e-300 else 0.0)
    assert worst > 3 * mes_ref.U          # (and it is a bound, not a zero)


def test_the_continued_fraction_truncates_below_a_quarter_rounding():
    """Depth 16 at |c| = 8, in exact arithmetic: both pieces that use it against the truth."""
    with mp.workdps(60):
        for x in (mp.mpf(8), mp.mpf(8) * (1 + mp.mpf(2) ** -30), mp.mpf(12), mp.mpf(100)):
            u = 1 / (x * x)
            b, a = mp.mpf(1), 1 + mes_ref.CF_K * u
            for k in range(mes_ref.CF_K - 1, 1, -1):
                a, b = a + k * u * b, a
            p1, p2, p3 = a + u * b, a, b
            left = mp.log(2 * mp.pi) / 2 - p3 / (2 * p2) + mp.log(x + p3 / p2 / x)
            t = mes_ref.g_truth(-x)
            assert abs(left - t) <= mes_ref.U / 4 * t, (x, float(abs(left - t) / t))
            right = mp.npdf(x) * (x / 2 + p2 / p1 / x)
            t = mes_ref.g_truth(x)
            assert abs(right - t) <= (3 * mes_ref.EPS + mes_ref.U / 4) * t, (x, float(abs(right - t) / t))


def test_sums_of_equal_samples_and_the_value_order():
    mu, s2 = np.array([0.3, -1.0, 2.0]), np.array([0.5, 1e-3, 4.0])
    one = mes.mes_value(mu, s2, [1.7])
    for S in (2, 4, 64):
        assert np.array_equal(mes.mes_value(mu, s2, [1.7] * S), one)
    ys = np.array([1.7, 2.1, 0.4, 3.3, 1.9, 2.6, 5.0])
    bad, worst = mes_ref.check_mes(mu, s2, ys, mes.mes_value(mu, s2, ys))
    assert not bad.any(), worst
    for wrong in (np.zeros(0), np.zeros(65), [np.nan], [np.inf]):
        with pytest.raises(ValueError, match='1 to 64 finite'):
            mes.mes_value(mu, s2, wrong)


# ---------------------------------------------------------------------------------------------------------------------
# the policy on the oracle's CPU model
# ---------------------------------------------------------------------------------------------------------------------
SEED, NGRID, NMAX, XI = 11, 400, 5, 0.01


def _model():
    rng = np.random.RandomState(3)
    X = rng.rand(12, 2)
    y = np.array([loop_objective(x) for x in X])
    gp = gp_ref.make_gp(1e-3, 0.5, [0.3, 0.35], float(y.mean()))
    gp.add_data(X, y)
    return gp, X


def test_the_gumbel_sampler_and_the_index():
    gp, X = _model()
    index = policies.MES(gp, BOUNDS2, X, nmax=NMAX, ngrid=NGRID, xi=XI, rng=SEED)
    kind, ystar = index.acq
    assert kind == 'mes' and ystar.shape == (NMAX,) and not hasattr(index, 'batch') and not hasattr(index, 'topk')
    # the same stream by hand: the support, its moments, the quartiles, the draws
    rng = np.random.RandomState(SEED)
    support = np.vstack([inits.init_uniform(BOUNDS2, NGRID, rng), X])
    mu, s2 = gp.predict(support)
    s = np.sqrt(s2)
    q = mes.gumbel_quantiles(mu, s)
    for level, y in zip((0.25, 0.5, 0.75), q):
        assert abs(np.sum(log_ndtr((y - mu) / s)) - np.log(level)) <= 1e-10
    b = (q[0] - q[2]) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    a = q[1] + b * np.log(np.log(2.0))
    assert b > 0.0
    floor = gp.predict(X)[0].max() + XI + 5.0 * np.sqrt(gp.sn2)
    want = np.maximum(a - b * np.log(-np.log(rng.rand(NMAX))), floor)
    assert np.allclose(ystar, want, rtol=0, atol=1e-12) and np.all(ystar >= floor)
    # floored draws stay floored: an xi that lifts the floor over every draw
    high = policies.MES(gp, BOUNDS2, X, nmax=NMAX, ngrid=NGRID, xi=50.0, rng=SEED).acq[1]
    assert np.all(high == gp.predict(X)[0].max() + 50.0 + 5.0 * np.sqrt(gp.sn2))
    # the index IS the reference closure on the model's moments, and that closure meets the bound
    Z = np.random.RandomState(4).rand(40, 2)
    mz, sz = gp.predict(Z)
    vals = index(Z)
    assert np.array_equal(vals, mes.mes_value(mz, sz, ystar)) and np.all(vals > 0.0)
    bad, worst = mes_ref.check_mes(mz, sz, ystar, vals)
    assert not bad.any(), worst
    # the caller's model is untouched by the policy (it works on a copy)
    assert gp.ndata == 12


def test_the_host_gradient_agrees_with_central_differences():
    """dMES/dx of the index against central differences of its own value at step h = 1e-6.  Tolerance, per component: what that step's
    truncation and rounding give for the reference itself, read off its own second differences -- |f(x + h) - 2 f(x) + f(x - h)| is
    h^2 |f''| plus four roundings of f, and divided by h it dominates both the central difference's truncation (h^2 |f'''| / 6) and its
    rounding (|df| / h) -- times 10, plus 10 eps |f| / h for a second difference that happens to vanish.  On this model the tolerance
    comes to 1e-6 .. 1e-3 of the gradient's size."""
    gp, X = _model()
    index = policies.MES(gp, BOUNDS2, X, nmax=NMAX, ngrid=NGRID, xi=XI, rng=SEED)
    Z = 0.1 + 0.8 * np.random.RandomState(6).rand(8, 2)
    f, G = index(Z, grad=True)
    assert np.array_equal(f, index(Z)) and G.shape == Z.shape
    h = 1e-6
    rel = []
    for j in range(2):
        e = np.zeros(2)
        e[j] = h
        fp, fm = index(Z + e), index(Z - e)
        fd = (fp - fm) / (2 * h)
        tol = 10 * np.abs(fp - 2 * f + fm) / h + 10 * mes_ref.EPS * np.abs(f) / h
        assert np.all(np.abs(G[:, j] - fd) <= tol), (j, np.abs(G[:, j] - fd) / tol)
        rel.append(tol / np.maximum(np.abs(G[:, j]), 1e-300))
    assert np.median(rel) < 1e-2          # (the check is not vacuous)


def test_solve_bayesopt_resolves_and_runs_mes():
    gp, _ = _model()
    grid = np.random.RandomState(7).rand(300, 2)
    xbest, model, info = pybo_amd.solve_bayesopt(loop_objective, BOUNDS2, model=gp, niter=5, policy=('mes', {'nmax': 4, 'ngrid': 200}),
                                                 solver=('lbfgs', {'xgrid': grid, 'nbest': 3}), recommender='incumbent', rng=0)
    assert info.x.shape == (6, 2) and model.ndata == 12 + 6 and np.all((info.x >= 0) & (info.x <= 1))
    assert np.all(np.isfinite(info.y)) and xbest.shape == (2,)


def test_batch_proposals_refuse_mes():
    gp, X = _model()
    with pytest.raises(ValueError, match='batch proposals need an EI, PI or UCB index'):
        pybo_amd.propose_batch(gp, BOUNDS2, X, 3, policy=('mes', {'nmax': 3, 'ngrid': 100}), xgrid=np.random.RandomState(1).rand(50, 2),
                               rng=0)


def test_an_ensemble_draws_one_set_per_member():
    """policies.MES on pybo_amd.models.MCMC-like ensembles: a stand-in with `members` and `get_entropy` (no device)."""
    gp, X = _model()
    other = gp_ref.make_gp(1e-3, 0.8, [0.2, 0.5], gp.bias)
    other.add_data(X, gp.Y)

    class Ens(object):
        def __init__(self, ms):
            self.members = ms

        def copy(self):
            return Ens([m.copy() for m in self.members])

        def get_entropy(self, ystar, Z, grad=False):
            return np.mean([mes.mes_value(*m.predict(Z), ys) for m, ys in zip(self.members, ystar)], axis=0)

    index = policies.MES(Ens([gp, other]), BOUNDS2, X, nmax=3, ngrid=100, rng=2)
    ystar = index.acq[1]
    assert ystar.shape == (2, 3) and not np.array_equal(ystar[0], ystar[1])
    Z = np.random.RandomState(8).rand(5, 2)
    want = 0.5 * (mes.mes_value(*gp.predict(Z), ystar[0]) + mes.mes_value(*other.predict(Z), ystar[1]))
    assert np.array_equal(index(Z), want)
