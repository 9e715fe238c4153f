"""Reference for batch proposals of the constrained index (gpx_constrained_sweep_batch, Constrained.acq_batch, the 'cei' path of
pybo_amd.propose_batch): a from-scratch greedy over oracle.gp_ref models, target and thresholds frozen.  The members are the
objective (where there is one) and the J constraints.  Every round REFITS each member on [X; picks] with that member's own believer
values (each pick observed at the posterior mean THAT member had for it when it was picked), predicts all of Z, forms the chain of
con_ref.py -- EI or PI of the objective folded with every constraint's probability of feasibility, v * min(p, 1); without an
objective the chain starts at 1 -- and takes the best candidate not picked yet (value descending, index ascending, NaN last).
Nothing of the device's recurrence is used here.

Problems: con_cases.problem(name, m=3001).  Admission as in batch_ref: every round's relative margin between the best and the
second-best value >= batch_ref.MIN_MARGIN, and distinct picks."""
import functools

import numpy as np

import batch_ref
from batch_ref import acq_from_moments
import con_cases
import con_ref
from oracle import gp_ref

M = 3001
# tag: con_cases name, acquisition of the objective (None: no objective, the probability of feasibility alone), nb
CASES = {
    'se_j2_ei': ('se_j2', 'ei', 8),
    'm5_j3_ei': ('m5_j3', 'ei', 8),
    'se_j1_pi': ('se_j1', 'pi', 8),
    'se_j1_ei_nb16': ('se_j1', 'ei', 16),
    'se_j2_n9_ei': ('se_j2_n9', 'ei', 4),
    'se_j2_pof': ('se_j2', None, 8),
}


def members_of(p, kind, n=None):
    """(hypers [(sn2, rho, ell, bias)], Y (n, members), params) of a con_cases problem's members in the device's order: the objective
    first where kind is not None (param: the target), then the constraints (params: the thresholds)."""
    n = len(p['X']) if n is None else n
    first = 0 if kind is not None else 1
    Y = np.column_stack([p['y'], p['C']])[:n, first:]
    return p['hypers'][first:], Y, ([] if kind is None else [target_of(p, kind)]) + list(p['thr'])


def target_of(p, kind):
    return None if kind is None else p['target'] + (0.05 if kind == 'pi' else 0.0)


def chain_value(kind, params, mus, s2s):
    """The constrained index from the members' moments (n, M), the objective first where kind is not None."""
    first = 0 if kind is None else 1
    ps = [con_ref.pi_from_moments(mu, s2, t) for mu, s2, t in zip(mus[first:], s2s[first:], params[first:])]
    if kind is None:
        return con_ref.pof_chain(ps)
    return con_ref.chain(acq_from_moments(kind, params[0], mus[0], s2s[0]), ps)


def greedy(X, Y, Z, kernel, hypers, kind, params, nb):
    """dict(idx, val, margin (nb,); mu, s2 (n, nb): every member's moments at the pick at the moment it was picked).  Y (N, n): column
    m the observations of member m; hypers, params per member."""
    n = len(hypers)
    Xa = np.array(X, dtype=float)
    ya = [np.array(Y[:, m], dtype=float) for m in range(n)]
    idx, val, margin, mup, s2p = [], [], [], [], []
    for j in range(nb):
        mus, s2s = [], []
        for m, (sn2, rho, ell, bias) in enumerate(hypers):
            gp = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
            gp.add_data(Xa, ya[m])
            mu, s2 = gp.predict(Z)
            mus.append(mu), s2s.append(s2)
        mus, s2s = np.array(mus), np.array(s2s)
        v = np.array(chain_value(kind, params, mus, s2s), dtype=float)
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


def val_tol(kind, params, hypers, mu, s2):
    """Tolerance of a pick's value at the reference's member moments mu, s2 (n, nb): the members' stated tolerances
    (test_gpu_batch.acq_tol: helpers.mu_tol / s2_tol through EI or PI) propagated to first order through the product exactly as
    con_ref.values does it -- |dv| <= da + a sum_j dP_j with every P_j <= 1, a = 1 and da = 0 without an objective -- plus con_ref.TINY."""
    from test_gpu_batch import acq_tol
    first = 0 if kind is None else 1
    dps = sum(acq_tol('pi', params[m], mu[m], s2[m], hypers[m][1]) for m in range(first, len(hypers)))
    if kind is None:
        return dps + con_ref.TINY
    a = acq_from_moments(kind, params[0], mu[0], s2[0])
    return acq_tol(kind, params[0], mu[0], s2[0], hypers[0][1]) + np.abs(a) * dps + con_ref.TINY


def greedy_of(p, kind, nb, n=None):
    """The greedy on a con_cases problem (its first n observations)."""
    n = len(p['X']) if n is None else n
    hypers, Y, params = members_of(p, kind, n)
    return greedy(p['X'][:n], Y, p['Z'], p['kernel'], hypers, kind, params, nb)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(problem, kind, nb, reference) of a named case; computed once per session and shared -- treat all of it as read-only."""
    name, kind, nb = CASES[tag]
    p = con_cases.problem(name, m=M)
    ref = greedy_of(p, kind, nb)
    for a in list(p.values()) + list(ref.values()) + [h[2] for h in p['hypers']]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p, kind, nb, ref


def admitted(ref):
    return bool(ref['margin'].min() >= batch_ref.MIN_MARGIN and len(set(ref['idx'].tolist())) == len(ref['idx']))
