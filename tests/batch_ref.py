"""Reference for batch proposals (gpx_sweep_batch, pybo_amd.propose_batch): a from-scratch greedy on oracle.gp_ref.  Every round
REFITS on [X; picks] with believer values (each pick observed at the posterior mean it had when it was picked), predicts all
of Z, scores with the frozen parameter and takes the best candidate not picked yet (value descending, index ascending, NaN
last).  Nothing of the device's recurrence (cached sums, cross terms) is used here.

A case is ADMITTED only if every round's relative margin between the best and the second-best value is >= MIN_MARGIN = 1e-5,
ten times the 1e-6 acquisition tolerance: a correct device cannot then legitimately pick differently."""
import functools

import numpy as np

from oracle import gp_ref
from helpers import synth_problem

MIN_MARGIN = 1e-5
RHO, SN2, BIAS = 1.3, 1e-3, 0.2

# tag: kernel, N, d, factor on the generated ell, acquisition, nb
CASES = {
    'se_300_3_ei': ('se', 300, 3, 1.0, 'ei', 8),
    'se_300_3_ei_nb24': ('se', 300, 3, 1.0, 'ei', 24),
    'matern5_256_2_ucb': ('matern5', 256, 2, 1.0, 'ucb', 8),
    'matern3_200_20_ei': ('matern3', 200, 20, 3.0, 'ei', 8),
    'matern1_130_5_pi': ('matern1', 130, 5, 1.0, 'pi', 8),
    'se_140_40_ucb': ('se', 140, 40, 4.0, 'ucb', 8),          # (ell unscaled: prior-dominated, margins ~1e-8 -- not usable)
}


def acq_from_moments(kind, param, mu, s2):
    if kind == 'ucb':
        return mu + np.sqrt(param * s2)
    s = np.sqrt(s2)
    z = (mu - param) / s
    if kind == 'pi':
        return gp_ref.norm_cdf(z)
    return (mu - param) * gp_ref.norm_cdf(z) + s * gp_ref.norm_pdf(z)


def greedy(X, y, Z, kernel, ell, rho, sn2, bias, kind, param, nb):
    """dict(idx (nb,), val (nb,), s2 (nb,), margin (nb,), mu_pick (nb,), mu_last, s2_last (M,): the moments that scored the last
    pick, i.e. conditioned on the first nb - 1)."""
    Xa, ya = np.array(X, dtype=float), np.array(y, dtype=float)
    idx, val, s2p, mup, margin = [], [], [], [], []
    for j in range(nb):
        gp = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
        gp.add_data(Xa, ya)
        mu, s2 = gp.predict(Z)
        v = acq_from_moments(kind, param, mu, s2)
        v = np.where(np.isnan(v), -np.inf, v)
        v[idx] = -np.inf                                  # (a picked candidate is excluded; its true value is not -inf)
        order = np.lexsort((np.arange(len(v)), -v))
        i, second = int(order[0]), int(order[1])
        vi = acq_from_moments(kind, param, mu[i], s2[i])
        idx.append(i), val.append(float(vi)), s2p.append(float(s2[i])), mup.append(float(mu[i]))
        margin.append(float((v[i] - v[second]) / abs(v[i])))
        Xa = np.vstack([Xa, Z[i:i + 1]])
        ya = np.hstack([ya, mu[i]])
    return dict(idx=np.array(idx, dtype=np.int64), val=np.array(val), s2=np.array(s2p), mu_pick=np.array(mup),
                margin=np.array(margin), mu_last=mu, s2_last=s2)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(problem, reference) of a named case; computed once per session and shared -- treat both as read-only."""
    kernel, N, d, fell, kind, nb = CASES[tag]
    X, y, ell = synth_problem(N, d, seed=17)
    ell = ell * fell
    Z = np.random.RandomState(5).rand(3001, d)
    base = gp_ref.make_gp(SN2, RHO, ell, BIAS, kernel)
    base.add_data(X, y)
    target = float(base.mean_at_obs().max())
    param = {'ei': target, 'pi': target + 0.05, 'ucb': 2.0}[kind]
    prob = dict(X=X, y=y, ell=ell, Z=Z, kernel=kernel, kind=kind, param=param, nb=nb, rho=RHO, sn2=SN2, bias=BIAS)
    ref = greedy(X, y, Z, kernel, ell, RHO, SN2, BIAS, kind, param, nb)
    for a in list(prob.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob, ref
