"""Reference for fantasised batch proposals (gpx_sweep_batch_fantasy, pybo_amd.propose_batch(..., fantasies=S)) on oracle.gp_ref.

Pending outcomes are integrated out by Monte Carlo (Snoek, Larochelle & Adams 2012, section 3.2): S joint fantasies of the picks'
observations, fantasy s observing  y_{s,l} = m_s(x_l) + sqrt(s2_l + sn2) eps[s][l]  at pick l, and every candidate scored by the
mean over s of EI / PI at its fantasy mean m_s against the fantasy's target t_s (incumbent 0: the caller's for the whole batch;
1: raised to the fantasy's posterior mean at each pick right after its own observation there).  Values are summed in fantasy order
and divided once by S; picks are value descending, index ascending, NaN last; `pending` rows are forced onto the leading rounds.

    greedy_refits       every round factorises [X; picks] from scratch and solves for every fantasy's own observations; nothing of
                        the device's recurrence (cached sums, cross terms, rows of V) is used
    greedy_recurrence   the recurrence itself in numpy on the oracle's exact posterior of the data: one covariance row per pick,
                        O(N M); for sizes where nb refits of a growing system would be too slow

Both return dict(idx, val, s2, margin (nb,); mu_pick, t (nb, S): every fantasy's mean at the pick and the target it was scored
against; vrow (nb - 1, M): v_l[n] = Cov(y_l, f(z_n) | data, picks < l) / d_l, what the tolerance of a fantasy mean is built from;
gain (nb - 1,): s2_l / d_l; s2_last (M,): the variances that scored the last pick).  A forced round's margin is +inf.

A case is ADMITTED only if every round's relative margin between the best and the second-best value is >= batch_ref.MIN_MARGIN."""
import functools

import numpy as np
import scipy.linalg as sla
from scipy.special import erfc

from oracle import gp_ref
from helpers import synth_problem, mu_tol, s2_tol

MIN_MARGIN = 1e-5
RHO, SN2, BIAS = 1.3, 1e-3, 0.2
EPS_SEED, EPS_COLS = 23, 63

# tag: kernel, N, d, factor on the generated ell, acquisition, S, nb
CASES = {
    'se_300_3_ei_s16': ('se', 300, 3, 1.0, 'ei', 16, 8),
    'matern5_256_2_pi_s8': ('matern5', 256, 2, 1.0, 'pi', 8, 6),
    'matern3_200_20_ei_s5': ('matern3', 200, 20, 3.0, 'ei', 5, 6),
    'matern1_130_5_ei_s64': ('matern1', 130, 5, 1.0, 'ei', 64, 8),
}


def _cdf(z):
    return 0.5 * erfc(-z * 0.70710678118654752440)


def _pdf(z):
    return 0.39894228040143267794 * np.exp(-0.5 * z * z)


def acq(kind, t, mu, s2):
    s = np.sqrt(s2)
    z = (mu - t) / s
    if kind == 'pi':
        return _cdf(z)
    assert kind == 'ei'
    return (mu - t) * _cdf(z) + s * _pdf(z)


def fantasy_value(kind, t, mu, s2):
    """mu (S, M), s2 (M,), t (S,): the sum over the fantasies in order from the first term, divided once."""
    acc = acq(kind, t[0], mu[0], s2)
    for s in range(1, len(mu)):
        acc = acc + acq(kind, t[s], mu[s], s2)
    return acc / float(len(mu))


def _pick(v, taken, forced):
    v = np.where(np.isnan(v), -np.inf, v)
    if forced is not None:
        return int(forced), np.inf
    v = v.copy()
    v[taken] = -np.inf
    order = np.lexsort((np.arange(len(v)), -v))
    i, second = int(order[0]), int(order[1])
    return i, float((v[i] - v[second]) / abs(v[i]))


def _result(idx, val, s2p, margin, mup, tt, vrow, gain, s2_last, nb, M):
    return dict(idx=np.array(idx, dtype=np.int64), val=np.array(val), s2=np.array(s2p), margin=np.array(margin), mu_pick=np.array(mup),
                t=np.array(tt), vrow=np.array(vrow).reshape(nb - 1, M), gain=np.array(gain), s2_last=s2_last)


def greedy_refits(X, y, Z, kernel, ell, rho, sn2, bias, kind, param, nb, eps, incumbent, pending=()):
    S, M = len(eps), len(Z)
    Xa = np.array(X, dtype=float)
    Ya = np.tile(np.array(y, dtype=float), (S, 1))                   # (S, N + picks): every fantasy's own observations
    t = np.full(S, float(param))
    idx, val, s2p, margin, mup, tt, vrow, gain = [], [], [], [], [], [], [], []
    for j in range(nb):
        gp = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
        gp.add_data(Xa, Ya[0])                                       # the factor is the same for every fantasy: K does not see y
        Ks = gp_ref.kernel(gp.kid, Xa, Z, gp.ell, rho)
        V = sla.solve_triangular(gp.L, Ks, lower=True)
        A = sla.solve_triangular(gp.L, (Ya - bias).T, lower=True)    # (N + j, S)
        mu = bias + (V.T @ A).T                                      # (S, M)
        s2 = np.maximum(rho - np.sum(V * V, axis=0), gp_ref.S2_FLOOR)
        if j and incumbent:
            t = np.maximum(t, mu[:, idx[-1]])                        # the mean at the last pick, its own observation absorbed
        v = fantasy_value(kind, t, mu, s2)
        i, mg = _pick(v, idx, pending[j] if j < len(pending) else None)
        idx.append(i), val.append(float(v[i])), s2p.append(float(s2[i])), margin.append(mg), mup.append(mu[:, i].copy()), tt.append(t.copy())
        if j + 1 < nb:
            dd = np.sqrt(s2[i] + sn2)
            kx = gp_ref.kernel(gp.kid, Z[i:i + 1], Z, gp.ell, rho)[0]
            vrow.append((kx - V[:, i] @ V) / dd)                     # Cov(y_j, f(z_n) | data, picks < j) / d_j
            gain.append(float(s2[i] / dd))
            Xa = np.vstack([Xa, Z[i:i + 1]])
            Ya = np.hstack([Ya, (mu[:, i] + dd * eps[:, j])[:, None]])
    return _result(idx, val, s2p, margin, mup, tt, vrow, gain, s2, nb, M)


def greedy_recurrence(X, y, Z, kernel, ell, rho, sn2, bias, kind, param, nb, eps, incumbent, pending=()):
    S, M = len(eps), len(Z)
    gp = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    gp.add_data(X, y)
    V0 = sla.solve_triangular(gp.L, gp_ref.kernel(gp.kid, gp.X, Z, gp.ell, rho), lower=True)
    mu0 = bias + V0.T @ gp.a
    q = np.sum(V0 * V0, axis=0)
    mu = np.tile(mu0, (S, 1))
    t = np.full(S, float(param))
    rows = np.zeros((0, M))
    idx, val, s2p, margin, mup, tt, gain = [], [], [], [], [], [], []
    for j in range(nb):
        s2 = np.maximum(rho - q, gp_ref.S2_FLOOR)
        v = fantasy_value(kind, t, mu, s2)
        i, mg = _pick(v, idx, pending[j] if j < len(pending) else None)
        idx.append(i), val.append(float(v[i])), s2p.append(float(s2[i])), margin.append(mg), mup.append(mu[:, i].copy()), tt.append(t.copy())
        if j + 1 == nb:
            break
        dd = np.sqrt(s2[i] + sn2)
        c = gp_ref.kernel(gp.kid, Z[i:i + 1], Z, gp.ell, rho)[0] - V0[:, i] @ V0 - rows[:, i] @ rows
        vj = c / dd
        if incumbent:
            t = np.maximum(t, mu[:, i] + (s2[i] / dd) * eps[:, j])
        gain.append(float(s2[i] / dd))
        rows = np.vstack([rows, vj])
        q = q + vj * vj
        mu = mu + np.outer(eps[:, j], vj)
    return _result(idx, val, s2p, margin, mup, tt, rows, gain, s2, nb, M)


def mean_slack(ref, eps, rho, j, col=None):
    """What a fantasy mean of round j may be off by, (S,): helpers.mu_tol plus, per pick l < j, |eps[s][l]| (1e-6 |v_l[n]| + 1e-9 sqrt(rho))
    -- a row of V is a covariance over d: the mean's tolerance per unit of it.  n = the round's pick, or `col`."""
    n = ref['idx'][j] if col is None else col
    coef = np.abs(ref['vrow'][:j, n])
    return mu_tol(ref['mu_pick'][j], rho) + np.abs(eps[:, :j]) @ (1e-6 * coef + 1e-9 * np.sqrt(rho))


def target_slack(ref, eps, rho, j):
    """The same for the targets of round j under incumbent 1, (S,): a target is a maximum of the caller's parameter (exact) and the u_{s,l},
    l < j, and a maximum is off by no more than the largest error of its terms.  u_{s,l} is a fantasy mean at pick l whose last
    coefficient is s2_l / d_l."""
    S = len(eps)
    out = np.zeros(S)
    for l in range(j):
        n = ref['idx'][l]
        coef = np.append(np.abs(ref['vrow'][:l, n]), ref['gain'][l])
        u = ref['mu_pick'][l] + ref['gain'][l] * eps[:, l]
        out = np.maximum(out, mu_tol(u, rho) + np.abs(eps[:, :l + 1]) @ (1e-6 * coef + 1e-9 * np.sqrt(rho)))
    return out


def value_tol(kind, ref, eps, rho, j, incumbent):
    """Tolerance of sel_val[j] from the reference's quantities alone: per fantasy the construction of test_gpu_batch.acq_tol (the moment
    tolerances to first order through the acquisition, plus 1e-6 relative) with the mean's tolerance widened by mean_slack and, under
    incumbent 1, the target's by target_slack through dEI/dt = -Phi(z) (PI: -phi(z) / s); averaged over the fantasies."""
    mu, t, s2 = ref['mu_pick'][j], ref['t'][j], ref['s2'][j]
    s = np.sqrt(s2)
    z = (mu - t) / s
    dmu = mean_slack(ref, eps, rho, j)
    dt = target_slack(ref, eps, rho, j) if incumbent else np.zeros(len(eps))
    if kind == 'ei':
        tol = 1e-6 * np.abs(acq('ei', t, mu, s2)) + 1.05 * (_cdf(z) * (dmu + dt) + _pdf(z) * s2_tol(s2, rho) / (2.0 * s))
    else:
        tol = 1e-6 * _cdf(z) + 1.05 * (_pdf(z) / s * (dmu + dt) + _pdf(z) * np.abs(z) / (2.0 * s2) * s2_tol(s2, rho))
    return float(np.mean(tol))


def eps_for(S, seed=EPS_SEED):
    return np.random.RandomState(seed).randn(S, EPS_COLS)


def problem(tag):
    kernel, N, d, fell, kind, S, nb = CASES[tag]
    X, y, ell = synth_problem(N, d, seed=17)
    ell = ell * fell
    Z = np.random.RandomState(5).rand(3001, d)
    base = gp_ref.make_gp(SN2, RHO, ell, BIAS, kernel)
    base.add_data(X, y)
    target = float(base.mean_at_obs().max())
    param = {'ei': target, 'pi': target + 0.05}[kind]
    return dict(X=X, y=y, ell=ell, Z=Z, kernel=kernel, kind=kind, param=param, nb=nb, S=S, eps=eps_for(S), rho=RHO, sn2=SN2, bias=BIAS)


def run(fn, prob, incumbent, nb=None, eps=None, pending=()):
    return fn(prob['X'], prob['y'], prob['Z'], prob['kernel'], prob['ell'], prob['rho'], prob['sn2'], prob['bias'], prob['kind'], prob['param'],
              prob['nb'] if nb is None else nb, prob['eps'] if eps is None else eps, incumbent, pending)


def _freeze(*dicts):
    for dct in dicts:
        for a in dct.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(tag, incumbent):
    """(problem, greedy_refits' result) of a named case; computed once per session and shared -- treat both as read-only."""
    prob = problem(tag)
    ref = run(greedy_refits, prob, incumbent)
    _freeze(prob, ref)
    return prob, ref


@functools.lru_cache(maxsize=None)
def case_recurrence(tag, incumbent):
    prob = problem(tag)
    ref = run(greedy_recurrence, prob, incumbent)
    _freeze(prob, ref)
    return prob, ref
