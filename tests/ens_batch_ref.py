"""Reference for batch proposals on the hyper-parameter ensemble (gpx_ensemble_sweep_batch, MCMC.acq_batch): a from-scratch
greedy over n oracle.gp_ref models, the members FROZEN.  Every round REFITS each member on [X; picks] with that member's own
believer values (each pick observed at the posterior mean THAT member had for it when it was picked), predicts all of Z, forms
the ensemble's value -- numpy's mean over the members for EI / PI, mixture moments mu = mean mu_m, s2 = max(mean(s2_m + mu_m^2)
- mu^2, 0), value mu + sqrt(beta s2) for UCB -- and takes the best candidate not picked yet (value descending, index ascending,
NaN last).  Nothing of the device's recurrence is used here.  With one member this is batch_ref.greedy.

Admission as in batch_ref: every round's relative margin between the best and the second-best value >= batch_ref.MIN_MARGIN."""
import functools

import numpy as np

import batch_ref
from batch_ref import RHO, SN2, BIAS, acq_from_moments
from oracle import gp_ref
from helpers import synth_problem

# tag: kernel, N, d, factor on the generated ell, acquisition, nb, members
CASES = {
    'se_300_3_ei_n3': ('se', 300, 3, 1.0, 'ei', 8, 3),
    'matern5_256_2_ucb_n4': ('matern5', 256, 2, 1.0, 'ucb', 8, 4),
    'matern3_200_20_ei_n3': ('matern3', 200, 20, 3.0, 'ei', 8, 3),
    'matern1_130_5_pi_n2': ('matern1', 130, 5, 1.0, 'pi', 8, 2),
    'se_140_40_ucb_n3': ('se', 140, 40, 4.0, 'ucb', 8, 3),
    'se_300_3_ei_nb16_n10': ('se', 300, 3, 1.0, 'ei', 16, 10),
    'se_140_260_ucb_n2': ('se', 140, 260, 10.0, 'ucb', 4, 2),      # d > 256: the pick kernel's gather takes a second step
}


def member_hypers(ell, n, rho=RHO, sn2=SN2, bias=BIAS):
    """[(ell_m, rho_m, sn2_m, bias_m)]: n members spread around a case's hyper-parameters (member 0 of n = 1 is the case itself)."""
    return [(ell * (1.0 + 0.15 * (m - (n - 1) / 2.0)), rho * (1.0 + 0.2 * m), sn2 * (1 + m), bias + 0.05 * m) for m in range(n)]


def ensemble_value(kind, param, mus, s2s):
    """The ensemble's value from the members' moments (n, M) -> (value (M,), mixture mu, mixture s2 [UCB only, else None])."""
    if kind == 'ucb':
        mu = np.mean(mus, axis=0)
        s2 = np.maximum(np.mean(s2s + mus ** 2, axis=0) - mu ** 2, 0.0)
        return mu + np.sqrt(param * s2), mu, s2
    return np.mean([acq_from_moments(kind, param, mu, s2) for mu, s2 in zip(mus, s2s)], axis=0), None, None


def greedy(X, y, Z, kernel, hypers, kind, param, nb):
    """dict(idx, val, margin (nb,); mu, s2 (n, nb): every member's moments at the pick at the moment it was picked)."""
    n = len(hypers)
    Xa = np.array(X, dtype=float)
    ya = [np.array(y, dtype=float) for _ in range(n)]
    idx, val, margin, mup, s2p = [], [], [], [], []
    for j in range(nb):
        mus, s2s = [], []
        for m, (ell, rho, sn2, bias) in enumerate(hypers):
            gp = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
            gp.add_data(Xa, ya[m])
            mu, s2 = gp.predict(Z)
            mus.append(mu), s2s.append(s2)
        mus, s2s = np.array(mus), np.array(s2s)
        v = ensemble_value(kind, param, mus, s2s)[0]
        vi_all = v.copy()
        v = np.where(np.isnan(v), -np.inf, v)
        v[idx] = -np.inf                                  # (a picked candidate is excluded; its true value is not -inf)
        order = np.lexsort((np.arange(len(v)), -v))
        i, second = int(order[0]), int(order[1])
        idx.append(i), val.append(float(vi_all[i])), mup.append(mus[:, i].copy()), s2p.append(s2s[:, i].copy())
        margin.append(float((v[i] - v[second]) / abs(v[i])))
        Xa = np.vstack([Xa, Z[i:i + 1]])
        ya = [np.hstack([ya[m], mus[m, i]]) for m in range(n)]
    return dict(idx=np.array(idx, dtype=np.int64), val=np.array(val), margin=np.array(margin), mu=np.array(mup).T.copy(),
                s2=np.array(s2p).T.copy())


def ensemble_param(X, y, kernel, hypers, kind):
    """EI: the largest mean over the members of their posterior means at the data; PI: that + 0.05; UCB: beta = 2."""
    if kind == 'ucb':
        return 2.0
    means = []
    for ell, rho, sn2, bias in hypers:
        gp = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
        gp.add_data(X, y)
        means.append(gp.mean_at_obs())
    target = float(np.mean(means, axis=0).max())
    return target if kind == 'ei' else target + 0.05


def problem(kernel, N, d, fell, kind, nb, n):
    X, y, ell = synth_problem(N, d, seed=17)
    ell = ell * fell
    Z = np.random.RandomState(5).rand(3001, d)
    hypers = member_hypers(ell, n)
    return dict(X=X, y=y, Z=Z, kernel=kernel, hypers=hypers, kind=kind, param=ensemble_param(X, y, kernel, hypers, kind), nb=nb)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(problem, reference) of a named case; computed once per session and shared -- treat both as read-only."""
    prob = problem(*CASES[tag])
    ref = greedy(prob['X'], prob['y'], prob['Z'], prob['kernel'], prob['hypers'], prob['kind'], prob['param'], prob['nb'])
    for a in list(prob.values()) + list(ref.values()) + [h[0] for h in prob['hypers']]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob, ref


def admitted(ref):
    return bool(ref['margin'].min() >= batch_ref.MIN_MARGIN and len(set(ref['idx'].tolist())) == len(ref['idx']))
