"""
Batch proposals: nb query points per model state, for objectives that evaluate in parallel.

The reference proposes one point per iteration (pybo/bayesopt.py:262-269); its only batch is q Thompson draws.
For EI / PI / UCB the standard answer is greedy hallucination (Kriging believer; GP-BUCB, Desautels et al. 2014): pick the
best candidate, condition the model on it with its value set to the current posterior mean -- the mean stays where it is,
only the variance shrinks -- and pick again, with the acquisition parameter (EI / PI target, UCB beta) frozen for the batch.

    propose_batch(model, bounds, X, nb, policy='ei', xgrid=None, ngrid=10000, rng=None) -> (Xq (nb, d), values (nb,), idx (nb,))

Three paths, chosen by what the policy's index carries:
  * `index.batch` (device models: `pybo_amd.models.GP`, and `pybo_amd.models.MCMC` over such members): every round runs on the
    GPU over the warm sweep cache (gpx_sweep_batch / gpx_ensemble_sweep_batch); one O(N M) pass per member and extra point, the
    model untouched.  The ensemble's members are FROZEN for the batch -- no chain step, no refit: each member is conditioned on a
    pick at its own posterior mean and the ensemble's index (mean of the members' EI / PI, mixture moments for UCB) is re-scored;
  * `index.acq` only (an MCMC ensemble over other members, ShardedGP, the oracle's GPRef, stubs): the generic host path below --
    score the grid, pick, `copy()` the model once and `add_data(x, predict(x)[0])` per round.  On an `MCMC` that `add_data`
    advances the chain: the hyper-parameters are RE-SAMPLED on the hallucinated observation every round, unlike the device path;
  * neither (Thompson, or any sampled policy): nb independent policy calls, each one's best grid point; duplicates are allowed.
`policy='mes'` is refused: its index carries `.acq = ('mes', ystar)` but no `.batch`, and `_score` below raises the ValueError for any kind
but EI, PI and UCB -- scoring the believer rounds with max-value entropy search is not built (the sampled maxima would have to follow them).
`policy='kg'` is refused the same way: `.acq = ('kg', support)`, no `.batch` (the support set's means would have to follow the rounds).
Picks are grid candidates, ranked value descending, then index ascending, NaN last -- the device top-k's order.
"""
import numpy as np

from . import inits
from .utils import rstate

__all__ = ['propose_batch']


def _rank_first(values, taken):
    v = np.where(np.isnan(values), -np.inf, np.asarray(values, dtype=float))
    order = np.lexsort((np.arange(len(v)), -v))
    return int(next(i for i in order if i not in taken))


def _score(model, kind, param, Z):
    if kind == 'ei':
        return model.get_improvement(param, Z)
    if kind == 'pi':
        return model.get_tail(param, Z)
    if kind == 'ucb':
        mu, s2 = model.predict(Z)
        return mu + np.sqrt(param * s2)
    raise ValueError('batch proposals need an EI, PI or UCB index, not %r' % (kind,))


def _host_batch(model, kind, param, Z, nb):
    """The generic path: any model with the protocol.  The caller's model is copied once and never touched."""
    work = model.copy()
    idx, vals = [], []
    for j in range(nb):
        v = _score(work, kind, param, Z)
        i = _rank_first(v, set(idx))
        idx.append(i)
        vals.append(float(v[i]) if not np.isnan(v[i]) else -np.inf)
        if j + 1 < nb:
            x = Z[i:i + 1]
            work.add_data(x, work.predict(x)[0])          # the believer: observe the posterior mean
    return np.array(vals), np.array(idx, dtype=np.int64)


def _propose(model, bounds, X, nb, policy, xgrid, ngrid, rng):
    """`policy`: already a callable policy(model, bounds, X) -> index."""
    nb = int(nb)
    if nb < 1:
        raise ValueError('nb must be at least 1')
    if xgrid is None:
        xgrid = inits.init_uniform(bounds, ngrid, rng)
    if nb > len(xgrid):
        raise ValueError('nb exceeds the number of grid points')
    index = policy(model, bounds, X)
    acq = getattr(index, 'acq', None)
    if acq is None:                                   # a sampled policy: one fresh index per point
        vals, idx = [], []
        for j in range(nb):
            if j:
                index = policy(model, bounds, X)
            topk = getattr(index, 'topk', None)
            if topk is not None:
                v, i = topk(xgrid, 1)
                vals.append(float(v[0]))
                idx.append(int(i[0]))
            else:
                v = np.asarray(index(np.asarray(xgrid)))
                i = _rank_first(v, ())
                vals.append(float(v[i]))
                idx.append(i)
        vals, idx = np.array(vals), np.array(idx, dtype=np.int64)
    elif getattr(index, 'batch', None) is not None:
        out = index.batch(xgrid, nb)
        vals, idx = np.asarray(out['sel_val']), np.asarray(out['sel_idx'], dtype=np.int64)
    else:
        vals, idx = _host_batch(model, acq[0], acq[1], np.asarray(xgrid, dtype=float), nb)
    return np.array(xgrid[idx], dtype=float).reshape(nb, -1), vals, idx


def propose_batch(model, bounds, X, nb, policy='ei', xgrid=None, ngrid=10000, rng=None):
    """nb points to evaluate next, given `model` and the points `X` observed so far: (Xq (nb, d), values (nb,), grid indices
    (nb,)).  `policy`: a name, a callable or (name-or-callable, kwargs), as in solve_bayesopt.  `xgrid`: the candidates -- an
    (M, d) array or a `DeviceGrid`; default `init_uniform(bounds, ngrid, rng)`.  The model is left as it was."""
    from . import policies
    from .bayesopt import get_component
    rng = rstate(rng)
    bounds = np.array(bounds, dtype=float, ndmin=2)
    return _propose(model, bounds, X, nb, get_component(policy, policies, rng), xgrid, ngrid, rng)
