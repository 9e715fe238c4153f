"""
Batch proposals: nb query points per model state, for objectives that evaluate in parallel.

The reference proposes one point per iteration (pybo/bayesopt.py:262-269); its only batch is q Thompson draws.
For EI / PI / UCB the standard answer is greedy hallucination (Kriging believer; GP-BUCB, Desautels et al. 2014): pick the
best candidate, condition the model on it with its value set to the current posterior mean -- the mean stays where it is,
only the variance shrinks -- and pick again, with the acquisition parameter (EI / PI target, UCB beta) frozen for the batch.

    propose_batch(model, bounds, X, nb, policy='ei', xgrid=None, ngrid=10000, rng=None, fantasies=0, incumbent='fantasy',
                  pending=None) -> (Xq (nb, d), values (nb,), idx (nb,))

Three paths, chosen by what the policy's index carries:
  * `index.batch` (device models: `pybo_amd.models.GP`, and `pybo_amd.models.MCMC` over such members): every round runs on the
    GPU over the warm sweep cache (gpx_sweep_batch / gpx_ensemble_sweep_batch); one O(N M) pass per member and extra point, the
    model untouched.  The ensemble's members are FROZEN for the batch -- no chain step, no refit: each member is conditioned on a
    pick at its own posterior mean and the ensemble's index (mean of the members' EI / PI, mixture moments for UCB) is re-scored;
  * `index.acq` only (an MCMC ensemble over other members, ShardedGP, the oracle's GPRef, stubs): the generic host path below --
    score the grid, pick, `copy()` the model once and `add_data(x, predict(x)[0])` per round.  On an `MCMC` that `add_data`
    advances the chain: the hyper-parameters are RE-SAMPLED on the hallucinated observation every round, unlike the device path;
  * neither (Thompson, or any sampled policy): nb independent policy calls, each one's best grid point; duplicates are allowed.
`policy='cei'` on a constrained model (`pybo_amd.models.Constrained`): its index carries `.acq = ('cei', target)` and never `.batch`, so
the dispatch is on the kind and the MODEL is asked.  One with `acq_batch` and device members on one device takes the device path
(gpx_constrained_sweep_batch: target and thresholds frozen, the objective AND every constraint conditioned on a pick at its own posterior
mean, one call for the whole batch); any other (oracle members, stubs) takes the generic host path, `_score` reading `get_constrained` and
the believer step observing EVERY member at its own posterior mean, a (1, 1 + J) row to `add_data`.  `fantasies > 0` or `pending` on a
constrained model raise a ValueError before any index is built (not built; nor are MCMC / ShardedGP members, off-grid refinement of the
picks, pruned seeding of the caches, or batches for MES and KG).
`policy='ehvi'` on a two-objective model (`pybo_amd.models.MultiObjective`) goes the same way: `.acq = ('ehvi', (front, ref))`, never
`.batch`.  Both members and `ref` are frozen and each member is conditioned on a pick at its own posterior mean; new here, THE FRONT FOLLOWS
THE PICKS: a believer leaves every pick's mean on or above the old front, so the pick's believed outcome `(mu_1(x), mu_2(x))` joins the front
before the next round (what it dominates leaves).  Device members: one call (gpx_ehvi_sweep_batch; the front is updated on the device);
others: the host path, `_score` reading `get_ehvi` over the grown front, a (1, 2) row to `add_data`.  `fantasies` / `pending`: ValueError.
`policy='mes'` is refused: its index carries `.acq = ('mes', ystar)` but no `.batch`, and `_score` below raises the ValueError for any kind
but EI, PI and UCB -- scoring the believer rounds with max-value entropy search is not built (the sampled maxima would have to follow them).
`policy='kg'` is refused the same way: `.acq = ('kg', support)`, no `.batch` (the support set's means would have to follow the rounds).
Picks are grid candidates, ranked value descending, then index ascending, NaN last -- the device top-k's order.

`fantasies=S > 0` (EI / PI on a single model) replaces the believer by Monte Carlo over the pending outcomes (Snoek, Larochelle &
Adams 2012, section 3.2; BoTorch's `X_pending`): S joint fantasies of the picks' observations, drawn from `eps = rng.randn(S, 63)`
(row s, column l: the standard-normal innovation of pick l under fantasy s), and every candidate scored by its EI / PI averaged
over them -- the mean moves with each fantasy, the variance shrinks as before.  `incumbent='fantasy'`: a fantasy's target follows
the posterior mean at its own fantasised observations (best posterior mean at the data, as the policies take it); `'fixed'`: the
policy's target for the whole batch.  `pending`: grid rows already being evaluated (asynchronous workers) -- the leading picks are
forced to them, the free picks integrate over their outcomes too.  Device models run it in gpx_sweep_batch_fantasy on the believer's
recurrence (no refit, no extra pass over the grid); any other single model with copy / add_data / predict takes `_host_fantasy`
below, which keeps S copies and lets copy s observe `mean_s(x) + sqrt(s2(x) + sn2) eps[s][l]` at pick l.  Ensembles (`models.MCMC`,
anything with `members`), `ShardedGP`, UCB (linear in the mean: its fantasy average is the believer's value), MES, KG and sampled
policies raise a ValueError.
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
    if kind == 'cei':                                 # a constrained model: EI times feasibility (param None: feasibility alone)
        return model.get_constrained(param, Z)
    if kind == 'ehvi' and getattr(model, 'get_ehvi', None) is not None:      # two objectives: param = (front, ref), the front AS IT STANDS
        return model.get_ehvi(param[0], param[1], Z)
    raise ValueError('batch proposals need an EI, PI or UCB index (or CEI on a constrained, EHVI on a two-objective model), not %r' % (kind,))


def _believe(work, kind, x):
    """What the believer observes at x: the posterior mean; on a constrained model EVERY member's own, a (1, 1 + J) row; on a
    two-objective model the (1, 2) row of both members' means."""
    if kind == 'cei':
        return np.array([[float(m.predict(x)[0][0]) for m in [work.objective] + list(work.constraints)]])
    if kind == 'ehvi':
        return np.array([[float(m.predict(x)[0][0]) for m in work.objectives]])
    return work.predict(x)[0]


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
            y = _believe(work, kind, x)
            work.add_data(x, y)                           # the believer: observe the posterior mean
            if kind == 'ehvi':                            # .. and the front follows the picks: the believed outcome joins it
                param = (np.vstack([np.asarray(param[0], dtype=float).reshape(-1, 2), y]), param[1])
    return np.array(vals), np.array(idx, dtype=np.int64)


MAX_NB = 64                                           # picks per call of the device path: eps is drawn for all of them


def _incumbent_mode(incumbent):
    modes = {'fantasy': 1, 'fixed': 0, 1: 1, 0: 0}
    if isinstance(incumbent, (bool, np.bool_)) or incumbent not in modes:
        raise ValueError("incumbent must be 'fantasy' or 'fixed', not %r" % (incumbent,))
    return modes[incumbent]


def _host_fantasy(model, kind, param, Z, nb, eps, incumbent, pending):
    """The generic path with fantasies: S copies of the model, copy s observing its own draw of every pick.  Values are summed in
    fantasy order and divided once by S, the device's association."""
    from .policies.simple import _noise
    S = len(eps)
    sn2 = _noise(model)
    works = [model.copy() for _ in range(S)]
    target = [param] * S
    idx, vals = [], []
    for j in range(nb):
        v = _score(works[0], kind, target[0], Z)
        for s in range(1, S):
            v = v + _score(works[s], kind, target[s], Z)
        v = v / float(S)
        i = int(pending[j]) if j < len(pending) else _rank_first(v, set(idx))
        idx.append(i)
        vals.append(float(v[i]) if not np.isnan(v[i]) else -np.inf)
        if j + 1 < nb:
            x = Z[i:i + 1]
            for s, work in enumerate(works):
                m, s2 = work.predict(x)
                work.add_data(x, m + np.sqrt(s2 + sn2) * eps[s][j])
                if incumbent:                           # best posterior mean at the data, the new point included
                    target[s] = max(target[s], float(work.predict(x)[0][0]))
    return np.array(vals), np.array(idx, dtype=np.int64)


def _fantasy_model(model, nb, fantasies):
    """The refusals that need no index (so none is built): the number of fantasies and of picks, ensembles, ShardedGP."""
    S = int(fantasies)
    if S < 1 or S > 64:
        raise ValueError('fantasies must be in [0, 64]')
    if nb > MAX_NB:
        raise ValueError('a fantasised batch holds at most %d points' % MAX_NB)
    if hasattr(model, 'members'):
        raise ValueError('fantasies are not supported on ensembles (models.MCMC): a single model only')
    from .models import ShardedGP
    if isinstance(model, ShardedGP):
        raise ValueError('fantasies are not supported on ShardedGP: a single-device model only')


def _fantasy_args(index, nb, npts, fantasies, incumbent, pending, rng):
    """(eps, incumbent 0 / 1, pending rows) of a fantasised batch, or the ValueError that names what is not built."""
    acq = getattr(index, 'acq', None)
    if acq is None:
        raise ValueError('fantasies need an EI or PI index, not a sampled policy')
    if acq[0] not in ('ei', 'pi'):
        raise ValueError('fantasies need an EI or PI index, not %r (UCB is linear in the mean: its fantasy average is the believer\'s '
                         'value; MES and KG are not built)' % (acq[0],))
    pend = np.zeros(0, dtype=np.int64) if pending is None else np.array(pending, dtype=np.int64).reshape(-1)
    if len(pend) >= nb or len(set(pend.tolist())) != len(pend) or np.any(pend < 0) or np.any(pend >= npts):
        raise ValueError('pending must hold fewer than nb distinct grid rows')
    mode = _incumbent_mode(incumbent)
    return rng.randn(int(fantasies), MAX_NB - 1), mode, pend


def _propose(model, bounds, X, nb, policy, xgrid, ngrid, rng, fantasies=0, incumbent='fantasy', pending=None):
    """`policy`: already a callable policy(model, bounds, X) -> index."""
    nb = int(nb)
    if nb < 1:
        raise ValueError('nb must be at least 1')
    if xgrid is None:
        xgrid = inits.init_uniform(bounds, ngrid, rng)
    if nb > len(xgrid):
        raise ValueError('nb exceeds the number of grid points')
    if hasattr(model, 'get_constrained') and (fantasies or pending is not None):
        raise ValueError('fantasies and pending points are not supported on constrained models (models.Constrained): believer picks only')
    if hasattr(model, 'get_ehvi') and (fantasies or pending is not None):
        raise ValueError('fantasies and pending points are not supported on two-objective models (models.MultiObjective): believer picks only')
    if fantasies:
        _fantasy_model(model, nb, fantasies)
    index = policy(model, bounds, X)
    acq = getattr(index, 'acq', None)
    if fantasies:
        eps, mode, pend = _fantasy_args(index, nb, len(xgrid), fantasies, incumbent, pending, rng)      # (after the grid draw)
        if getattr(index, 'batch', None) is not None:
            out = index.batch(xgrid, nb, eps=eps, incumbent=mode, pending=pend if len(pend) else None)
            vals, idx = np.asarray(out['sel_val']), np.asarray(out['sel_idx'], dtype=np.int64)
        else:
            vals, idx = _host_fantasy(model, acq[0], acq[1], np.asarray(xgrid, dtype=float), nb, eps, mode, pend)
    elif pending is not None:
        raise ValueError('pending points need fantasies > 0')
    elif acq is None:                                 # a sampled policy: one fresh index per point
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
    elif acq[0] == 'cei' and getattr(model, 'acq_batch', None) is not None and getattr(model, '_device_members', lambda: False)():
        out = model.acq_batch('cei', acq[1], xgrid, nb)      # (the CEI index carries no `.batch`: the model is asked)
        vals, idx = np.asarray(out['sel_val']), np.asarray(out['sel_idx'], dtype=np.int64)
    elif acq[0] == 'ehvi' and getattr(model, 'acq_batch', None) is not None and getattr(model, '_device_members', lambda: False)():
        out = model.acq_batch('ehvi', acq[1], xgrid, nb)     # (nor does the EHVI index: the model is asked)
        vals, idx = np.asarray(out['sel_val']), np.asarray(out['sel_idx'], dtype=np.int64)
    elif getattr(index, 'batch', None) is not None:
        out = index.batch(xgrid, nb)
        vals, idx = np.asarray(out['sel_val']), np.asarray(out['sel_idx'], dtype=np.int64)
    else:
        vals, idx = _host_batch(model, acq[0], acq[1], np.asarray(xgrid, dtype=float), nb)
    return np.array(xgrid[idx], dtype=float).reshape(nb, -1), vals, idx


def propose_batch(model, bounds, X, nb, policy='ei', xgrid=None, ngrid=10000, rng=None, fantasies=0, incumbent='fantasy',
                  pending=None):
    """nb points to evaluate next, given `model` and the points `X` observed so far: (Xq (nb, d), values (nb,), grid indices
    (nb,)).  `policy`: a name, a callable or (name-or-callable, kwargs), as in solve_bayesopt.  `xgrid`: the candidates -- an
    (M, d) array or a `DeviceGrid`; default `init_uniform(bounds, ngrid, rng)`.  The model is left as it was.
    `fantasies=S > 0`: integrate over the picks' outcomes with S joint fantasies instead of believing their means (EI / PI, a single
    model; the normals are drawn from `rng` after the grid); `incumbent`: 'fantasy' or 'fixed'; `pending`: grid rows already being
    evaluated, returned as the leading picks (the module's docstring)."""
    from . import policies
    from .bayesopt import get_component
    rng = rstate(rng)
    bounds = np.array(bounds, dtype=float, ndmin=2)
    return _propose(model, bounds, X, nb, get_component(policy, policies, rng), xgrid, ngrid, rng, fantasies, incumbent, pending)
