"""
Two competing objectives behind ONE object with the model protocol, for black boxes that return `(f1(x), f2(x))`, both maximised
(the reference has nothing like it).  Each objective has its own model and hyper-parameters; the posteriors are taken as independent,
for which the expected hypervolume improvement over a Pareto front is exact and closed-form (pybo_amd/pareto.py; Emmerich et al. 2011,
Yang et al. 2019).  With device members (`pybo_amd.models.GP` on one device) the whole-grid index and its top-k are one call into the
library (gpx_ehvi_sweep[_dev]: `acq_topk`) and the moments and gradients of both members at a few points are one call too
(gpx_ensemble_predict: `get_ehvi`), and so are nb greedy batch picks over the members' warm sweep caches (gpx_ehvi_sweep_batch:
`acq_batch`, for `pybo_amd.propose_batch`); any other members (a test oracle, a stub) go through their `predict`.  Host logic only.
"""
import numpy as np

from .. import _lib, pareto
from .._lib import DeviceGrid
from .gp import GP

__all__ = ['MultiObjective']


class MultiObjective(object):
    def __init__(self, f1, f2):
        self.objectives = [f1, f2]

    # -- bookkeeping ---------------------------------------------------------------------------
    def copy(self):
        return MultiObjective(*[m.copy() for m in self.objectives])

    @property
    def ndata(self):
        return self.objectives[0].ndata

    @property
    def data(self):
        """(X, Y) with Y (n, 2): the columns as `add_data` takes them."""
        cols = [m.data for m in self.objectives]
        return cols[0][0], np.column_stack([c[1] for c in cols])

    def add_data(self, X, Y):
        """Y is (n, 2), columns [f1, f2] (one point: (2,)): what `objective(x)` returns in solve_bayesopt."""
        Y = np.array(Y, dtype=float)
        if Y.ndim < 2:
            Y = Y.reshape(-1, 2)
        if Y.shape[1] != 2:
            raise ValueError('Y must have 2 columns: one per objective')
        for j, m in enumerate(self.objectives):
            m.add_data(X, Y[:, j])

    def anticipate(self, x):
        started = False
        for m in self.objectives:
            ahead = getattr(m, 'anticipate', None)
            if ahead is not None:
                started = bool(ahead(x)) or started
        return started

    def predict_mean(self, X):
        """(n, 2): the posterior means of both objectives at the rows of X."""
        cols = []
        for m in self.objectives:
            mean_only = getattr(m, 'predict_mean', None)
            cols.append(np.asarray(mean_only(X) if mean_only is not None else m.predict(X)[0], dtype=float))
        return np.column_stack(cols)

    def pareto_set(self, X):
        """The rows of X whose posterior means no other row's dominate."""
        X = np.array(X, ndmin=2, dtype=float)
        return X[pareto.pareto_mask(self.predict_mean(X))]

    # -- the index -----------------------------------------------------------------------------
    def _device_members(self):
        ms = self.objectives
        return all(isinstance(m, GP) for m in ms) and len({int(m.device) for m in ms}) == 1

    def get_ehvi(self, front, ref, X, grad=False):
        """Expected hypervolume improvement over the raw points `front` (np, 2) above `ref` (2) at the rows of X [and its gradient,
        product rule on the host].  Device members: ONE gpx_ensemble_predict for the moments of both."""
        X = np.array(X, ndmin=2, dtype=float)
        a, b = pareto.strips(front, ref)
        if self._device_members() and len(X):
            mu, s2, dmu, ds2 = _lib.Engine.ensemble_predict([m._engine() for m in self.objectives], X)
            moms = [(mu[j], s2[j], dmu[j], ds2[j]) for j in range(2)]
        else:
            moms = [m.predict(X, True) for m in self.objectives] if grad else [tuple(m.predict(X)) + (None, None) for m in self.objectives]
        (m1, v1, dm1, dv1), (m2, v2, dm2, dv2) = moms
        return pareto.ehvi_from_moments(m1, v1, m2, v2, a, b, (dm1, dv1, dm2, dv2) if grad else None)

    def acq_topk(self, kind, param, xgrid, k):
        """Whole-grid EHVI + top-k on the device (gpx_ehvi_sweep[_dev]): (values (k,), grid indices (k,)).  kind 'ehvi', param =
        (front, ref).  Device `GP` members on one device; `xgrid` a DeviceGrid or a host array."""
        if kind != 'ehvi':
            raise ValueError("MultiObjective.acq_topk takes 'ehvi', not %r" % (kind,))
        if not self._device_members():
            raise TypeError('MultiObjective.acq_topk needs device GP members on one device')
        front, ref = param
        f1, f2 = [m._engine() for m in self.objectives]
        if isinstance(xgrid, DeviceGrid) and int(xgrid.device) != int(f1.device):
            xgrid = np.asarray(xgrid)                # resident on ANOTHER GPU: through the host, never its pointer
        if not isinstance(xgrid, DeviceGrid):
            xgrid = np.array(xgrid, ndmin=2, dtype=float)
        out = _lib.Engine.ehvi_sweep(f1, f2, front, ref, xgrid, k=int(k), want_all=False)
        self._lead = f1
        return out['top_val'], out['top_idx']

    def acq_batch(self, kind, param, xgrid, nb):
        """nb grid points to evaluate in parallel, on the device (gpx_ehvi_sweep_batch): greedy picks of EHVI with both members and the
        reference point frozen, each member conditioned on a pick at its own posterior mean and the pick's believed outcome -- the two
        means there -- taken into the front before the next round.  kind 'ehvi', param = (front, ref).  Each member's sweep cache is brought
        onto `xgrid` first (`GP._cache_grid`: a `DeviceGrid` that member's state has swept before is re-used, anything else is swept once
        with the cache on).  Returns dict(sel_val (nb,), sel_idx (nb,), sel_s2 (2, nb), sel_y (nb, 2), sel_nfront (nb,)).
        Not built: fantasised or pending picks, MCMC / ShardedGP members, off-grid refinement, pruned seeding, a moving reference point."""
        if kind != 'ehvi':
            raise ValueError("MultiObjective.acq_batch takes 'ehvi', not %r" % (kind,))
        if not self._device_members():
            raise TypeError('MultiObjective.acq_batch needs device GP members on one device')
        front, ref = param
        if not isinstance(xgrid, DeviceGrid) or int(xgrid.device) != int(self.objectives[0].device):
            xgrid = np.array(xgrid, ndmin=2, dtype=float)        # one host copy for both members
        f1, f2 = [m._cache_grid('ei', float(ref[j]), xgrid) for j, m in enumerate(self.objectives)]
        return _lib.Engine.ehvi_batch(f1, f2, front, ref, int(nb))

    def topk_engine(self):
        """The device handle whose HBM holds the (value, index) pairs of the last `acq_topk`: the first objective's."""
        lead = getattr(self, '_lead', None)
        return lead if lead is not None else self.objectives[0]._engine()
