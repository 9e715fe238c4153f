"""Reference for batch proposals of the two-objective index (gpx_ehvi_sweep_batch, MultiObjective.acq_batch, the 'ehvi' path of
pybo_amd.propose_batch): a from-scratch greedy over oracle.gp_ref models, both members and the reference point frozen.  Every round REFITS
both members on [X; picks] with that member's own believed values (each pick observed at the posterior mean THAT member had for it when it
was picked), predicts all of Z, builds the strips from scratch with ehvi_ref.strips(P + believed outcomes, ref), takes the values from
ehvi_ref.ehvi and picks the best candidate not picked yet (value descending, index ascending, NaN last).  Nothing of the device's
recurrence, and nothing of its front insertion, is used here.

Problems: ehvi_cases.problem(name, m=3001), N = 300.  Fronts: 'means' (the oracle's posterior means at X over ref = F.min(0) - 0.1 span),
'empty' (no points, the same ref), 'stairK' (ehvi_cases.raw_front(K, 3) between F.min() and F.max() with the ref it returns), 'highref' (no
points, ref 0.05 above every posterior mean over Z and X: no believed outcome ever enters the front).

Admission, on the reference alone: distinct picks; every round's relative margin between the best and the second-best value >=
batch_ref.MIN_MARGIN; and in each objective every coordinate among {the front's points, the believed outcomes, ref} separated from its
neighbours by >= 10 helpers.mu_tol -- means that differ from the oracle's within their tolerance then leave the front's membership and
order as they are."""
import functools

import numpy as np

import batch_ref
import ehvi_cases
import ehvi_ref
from helpers import mu_tol

M = 3001
# tag: (ehvi_cases name, front, nb, observations used)
CASES = {
    'se_d8_means': ('se_d8', 'means', 8, 300),
    'se_d8_empty': ('se_d8', 'empty', 8, 300),
    'se_d8_stair16': ('se_d8', 'stair16', 8, 300),
    'm5_d6_means': ('m5_d6', 'means', 8, 300),
    'm5_d6_empty': ('m5_d6', 'empty', 8, 300),
    'm5_d6_stair16': ('m5_d6', 'stair16', 8, 300),
    'm5_d6_stair256': ('m5_d6', 'stair256', 8, 300),
    'se_d8_stair1021': ('se_d8', 'stair1021', 4, 300),
    'm5_d6_stair1021': ('m5_d6', 'stair1021', 4, 300),
    'se_d8_highref': ('se_d8', 'highref', 8, 300),
    'm5_d6_highref': ('m5_d6', 'highref', 8, 300),
    'se_d8_means_n257': ('se_d8', 'means', 8, 257),
    'm5_d6_means_n257': ('m5_d6', 'means', 8, 257),
}
# the size of the front that scored each pick, as the issue that asked for this form recorded it
N_PER_ROUND = {
    'se_d8_means': [10, 9, 6, 6, 6, 7, 7, 7],
    'se_d8_empty': [0, 1, 2, 3, 4, 4, 4, 5],
    'se_d8_stair16': [16, 3, 4, 3, 4, 4, 4, 5],
    'm5_d6_means': [10, 10, 11, 11, 11, 11, 11, 11],
    'm5_d6_empty': [0, 1, 2, 3, 4, 4, 5, 5],
    'm5_d6_stair16': [16, 5, 3, 3, 4, 4, 4, 5],
    'm5_d6_stair256': [256, 68, 30, 30, 31, 15, 15, 15],
    'se_d8_stair1021': [1021, 120, 121, 3],
    'm5_d6_stair1021': [1021, 267, 115, 115],
    'se_d8_highref': [0] * 8,
    'm5_d6_highref': [0] * 8,
    'se_d8_means_n257': [9, 8, 7, 5, 6, 6, 6, 7],
    'm5_d6_means_n257': [11] + [12] * 7,
}


def front_of(p, how, n=None):
    """(P (np, 2), ref (2,)) of a named front on an ehvi_cases problem (its first n observations)."""
    n = len(p['X']) if n is None else n
    ms = ehvi_ref.models(p, n)
    F = np.column_stack([m.predict(p['X'][:n])[0] for m in ms])
    ref = F.min(0) - 0.1 * (F.max(0) - F.min(0))
    if how == 'means':
        return F, ref
    if how == 'empty':
        return np.empty((0, 2)), ref
    if how == 'highref':
        top = np.maximum(F.max(0), np.array([m.predict(p['Z'])[0].max() for m in ms]))
        return np.empty((0, 2)), top + 0.05
    assert how.startswith('stair')
    return ehvi_cases.raw_front(int(how[5:]), 3, lo=F.min(), hi=F.max())


def greedy(p, P, ref, nb, n=None):
    """dict(idx, val, margin, n (nb,); mom (nb, 4): mu1, s2_1, mu2, s2_2 at the pick when it was picked; y (nb, 2) the believed outcomes;
    strips [(a, b)] that scored each pick; P, ref) on the first n observations of p."""
    n = len(p['X']) if n is None else n
    Z = p['Z']
    Xa = np.array(p['X'][:n], dtype=float)
    ya = [np.array(p['Y'][:n, j], dtype=float) for j in range(2)]
    P = np.asarray(P, dtype=float).reshape(-1, 2)
    idx, val, margin, nf, mom, ys, strips = [], [], [], [], [], [], []
    for j in range(nb):
        moms = []
        for m in range(2):
            moms += list(ehvi_ref.fit(p['hypers'][m], p['kernels'][m], Xa, ya[m]).predict(Z))
        a, b = ehvi_ref.strips(np.vstack([P] + [np.array(ys).reshape(-1, 2)]), ref)
        v_all = np.array(ehvi_ref.ehvi(*moms, a, b), dtype=float)
        v = np.where(np.isnan(v_all), -np.inf, v_all)
        v[idx] = -np.inf                                  # (a picked candidate is excluded; its true value is not -inf)
        order = np.lexsort((np.arange(len(v)), -v))
        i, second = int(order[0]), int(order[1])
        idx.append(i), val.append(float(v_all[i])), nf.append(len(b) - 1), strips.append((a, b))
        margin.append(float((v[i] - v[second]) / abs(v[i])))
        mom.append([float(q[i]) for q in moms])
        ys.append([mom[-1][0], mom[-1][2]])
        Xa = np.vstack([Xa, Z[i:i + 1]])
        ya = [np.hstack([ya[m], ys[-1][m]]) for m in range(2)]
    return dict(idx=np.array(idx, dtype=np.int64), val=np.array(val), margin=np.array(margin), n=np.array(nf, dtype=np.int64),
                mom=np.array(mom), y=np.array(ys), strips=strips, P=P, ref=np.asarray(ref, dtype=float))


def separation(p, r):
    """The smallest gap between neighbouring coordinates of {the front's points, the believed outcomes, ref} over the tolerance of a mean
    there (helpers.mu_tol), the smaller of the two objectives."""
    worst = np.inf
    for c in range(2):
        x = np.sort(np.concatenate([ehvi_ref.front(r['P'], r['ref'])[:, c], r['y'][:, c], r['ref'][c:c + 1]]))
        gap = np.diff(x)
        tol = np.maximum(mu_tol(x[1:], p['hypers'][c][1]), mu_tol(x[:-1], p['hypers'][c][1]))
        worst = min(worst, float((gap / tol).min()))
    return worst


def admitted(p, r):
    return bool(len(set(r['idx'].tolist())) == len(r['idx']) and r['margin'].min() >= batch_ref.MIN_MARGIN and separation(p, r) >= 10.0)


def strips_vec(P, r):
    """ehvi_ref.strips by the same definition with the quadratic test as one numpy expression (the tolerance below rebuilds the strips
    4 j times per pick; test_ehvi_batch_cpu.py holds this twin against ehvi_ref.strips exactly)."""
    P = np.asarray(P, dtype=float).reshape(-1, 2)
    P = np.unique(P[(P[:, 0] > r[0]) & (P[:, 1] > r[1])], axis=0)
    ge = (P[:, None, 0] >= P[None, :, 0]) & (P[:, None, 1] >= P[None, :, 1])      # [q, p]: q weakly dominates p
    F = P[~(ge & ~np.eye(len(P), dtype=bool)).any(axis=0)]
    return np.concatenate([[r[0]], F[:, 0], [np.inf]]), np.concatenate([F[:, 1], [r[1]]])


class _At(object):
    """What ehvi_ref.values reads of a model, standing at recorded moments."""
    def __init__(self, rho, mu, s2):
        self.rho, self._m = rho, (np.atleast_1d(mu), np.atleast_1d(s2))

    def predict(self, Z):
        return self._m


def val_tol(p, r):
    """(nb,) tolerance of the picks' values: ehvi_ref.values' own at the reference's moments at the pick (the members' stated tolerances,
    each moment moved by its own, one at a time, times 1.05, plus 1e-6 of the cancelled magnitude) plus the first-order effect of the strips:
    every believed coordinate inserted so far moved by its helpers.mu_tol, one at a time, the strips rebuilt, the absolute changes of the
    value added with the same factor 1.05."""
    rhos = [h[1] for h in p['hypers']]
    front0 = np.column_stack([r['strips'][0][0][1:-1], r['strips'][0][1][:-1]])      # the front of P: what P's other points cannot change
    out = []
    for j, (mom, (a, b)) in enumerate(zip(r['mom'], r['strips'])):
        v, tol, _ = ehvi_ref.values([_At(rhos[0], mom[0], mom[1]), _At(rhos[1], mom[2], mom[3])], a, b, None)
        extra = 0.0
        for l in range(j):
            for c in range(2):
                moved = r['y'][:j].copy()
                moved[l, c] += mu_tol(moved[l, c], rhos[c])
                extra += abs(float(ehvi_ref.ehvi(*mom, *strips_vec(np.vstack([front0, moved]), r['ref']))[0]) - float(v[0]))
        out.append(float(tol[0]) + 1.05 * extra)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(problem, P, ref, nb, n_obs, reference) of a named case; computed once per session and shared -- treat all of it as read-only."""
    name, how, nb, n = CASES[tag]
    p = ehvi_cases.problem(name, m=M)
    P, ref = front_of(p, how, n)
    r = greedy(p, P, ref, nb, n)
    for arr in list(p.values()) + list(r.values()) + [h[2] for h in p['hypers']] + [P, ref]:
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return p, P, ref, nb, n, r
