"""
Constrained optimisation: an objective model and J constraint models behind ONE object with the model protocol, for black boxes
that return `(f(x), c_1(x), .., c_J(x))` where feasibility means `c_j(x) >= thresholds[j]` and every c_j is only known through its
noisy evaluations (Gardner et al. 2014; Gelbart et al. 2014).  The reference has nothing like it.

    cEI(x) = EI_f(x; target) * prod_j Pr(c_j(x) >= t_j)

The factors are independent GPs, each with its own hyper-parameters.  With device members (`pybo_amd.models.GP` on one device) the
whole-grid product and its top-k are one call into the library (gpx_constrained_sweep_dev: `acq_topk`), and moments and gradients of
all 1 + J members at a few points are one call too (gpx_ensemble_predict: `get_constrained`), and so are nb greedy batch picks over the
members' warm sweep caches (gpx_constrained_sweep_batch: `acq_batch`, for `pybo_amd.propose_batch`); with any other members (a test oracle,
a stub) the same arithmetic runs through their `get_improvement` / `get_tail`.  Host logic only: no GP arithmetic lives here.
"""
import numpy as np
from scipy.special import erfc

from .. import _lib
from .._lib import DeviceGrid
from .gp import GP

__all__ = ['Constrained']


def _fold(v, p):
    """One factor of the product as the device folds it (csrc/acq_core.h: con_fold): v * min(p, 1), a NaN p kept."""
    p = np.asarray(p, dtype=float)
    return v * np.where(p > 1.0, 1.0, p)


class Constrained(object):
    def __init__(self, objective, constraints, thresholds=0.0):
        self.objective = objective
        self.constraints = list(constraints)
        if not self.constraints:
            raise ValueError('Constrained needs at least one constraint model')
        self.thresholds = np.array(np.broadcast_to(np.asarray(thresholds, dtype=float), (len(self.constraints),)), dtype=float)
        if not np.all(np.isfinite(self.thresholds)):
            raise ValueError('the thresholds must be finite')

    # -- bookkeeping ---------------------------------------------------------------------------
    @property
    def _members(self):      # (not `members`: that name marks a hyper-parameter ensemble for the MES / KG policies)
        return [self.objective] + self.constraints

    def copy(self):
        return Constrained(self.objective.copy(), [c.copy() for c in self.constraints], self.thresholds.copy())

    @property
    def ndata(self):
        return self.objective.ndata

    @property
    def data(self):
        """(X, Y) with Y (n, 1 + J): the columns as `add_data` takes them."""
        cols = [m.data for m in self._members]
        return cols[0][0], np.column_stack([c[1] for c in cols])

    def add_data(self, X, Y):
        """Y is (n, 1 + J), columns [objective, c_1 .. c_J] (one point: (1 + J,)): what `objective(x)` returns in solve_bayesopt."""
        nm = 1 + len(self.constraints)
        Y = np.array(Y, dtype=float)
        if Y.ndim < 2:
            Y = Y.reshape(-1, nm)
        if Y.shape[1] != nm:
            raise ValueError('Y must have %d columns: the objective and %d constraints' % (nm, nm - 1))
        for j, m in enumerate(self._members):
            m.add_data(X, Y[:, j])

    def anticipate(self, x):
        started = False
        for m in self._members:
            ahead = getattr(m, 'anticipate', None)
            if ahead is not None:
                started = bool(ahead(x)) or started
        return started

    def predict(self, X, grad=False):
        return self.objective.predict(X, grad)

    def predict_mean(self, X, grad=False):
        mean_only = getattr(self.objective, 'predict_mean', None)
        if mean_only is not None:
            return mean_only(X, grad) if grad else mean_only(X)
        post = self.objective.predict(X, grad)
        return (post[0], post[2]) if grad else post[0]

    # -- the index -----------------------------------------------------------------------------
    def _device_members(self):
        ms = self._members
        return all(isinstance(m, GP) for m in ms) and len({int(m.device) for m in ms}) == 1

    def _member_terms(self, target, X):
        """Per member (value, gradient) at the rows of X: EI of the objective (None where target is None), then every constraint's
        probability of feasibility.  Device members: ONE gpx_ensemble_predict for all moments, the closed forms on the host."""
        X = np.array(X, ndmin=2, dtype=float)
        if self._device_members() and len(X):
            ms = self._members if target is not None else self.constraints
            mu, s2, dmu, ds2 = _lib.Engine.ensemble_predict([m._engine() for m in ms], X)
            ts = ([float(target)] if target is not None else []) + list(self.thresholds)
            terms = []
            for i, t in enumerate(ts):
                s = np.sqrt(s2[i])
                z = (mu[i] - t) / s
                cdf = 0.5 * erfc(-z * 0.70710678118654752440)
                pdf = 0.39894228040143267794 * np.exp(-0.5 * z * z)
                if target is not None and i == 0:
                    terms.append(((mu[i] - t) * cdf + s * pdf, cdf[:, None] * dmu[i] + (0.5 * pdf / s)[:, None] * ds2[i]))
                else:
                    terms.append((cdf, pdf[:, None] * (dmu[i] / s[:, None] - (0.5 * z / s2[i])[:, None] * ds2[i])))
            return ([None] if target is None else []) + terms
        first = None if target is None else self.objective.get_improvement(target, X, True)
        return [first] + [c.get_tail(t, X, True) for c, t in zip(self.constraints, self.thresholds)]

    def feasibility(self, X, grad=False):
        """prod_j Pr(c_j(x) >= t_j) at the rows of X [and its gradient]."""
        return self.get_constrained(None, X, grad)

    def get_constrained(self, target, X, grad=False):
        """EI of the objective over `target` times the probability of feasibility, folded in constraint order as the device folds
        it; target = None: the probability of feasibility alone.  With `grad` also the gradient (product rule on the host)."""
        X = np.array(X, ndmin=2, dtype=float)
        if not grad:
            v = 1.0 if target is None else self.objective.get_improvement(target, X)
            for c, t in zip(self.constraints, self.thresholds):
                v = _fold(v, c.get_tail(t, X))
            return np.asarray(v, dtype=float)
        terms = self._member_terms(target, X)
        if terms[0] is None:
            v, g = np.ones(len(X)), np.zeros(X.shape)
        else:
            v, g = np.array(terms[0][0], dtype=float), np.array(terms[0][1], dtype=float)
        for p, dp in terms[1:]:
            g = g * _fold(1.0, p)[:, None] + v[:, None] * np.where(p > 1.0, 0.0, 1.0)[:, None] * dp
            v = _fold(v, p)
        return v, g

    def acq_topk(self, kind, target, xgrid, k):
        """Whole-grid constrained index + top-k on the device (gpx_constrained_sweep[_dev]): (values (k,), grid indices (k,)).  kind
        'cei': EI of the objective times the feasibility (target = None: feasibility alone).  Device `GP` members on one device;
        `xgrid` a DeviceGrid or a host array."""
        if kind != 'cei':
            raise ValueError("Constrained.acq_topk takes 'cei', not %r" % (kind,))
        if not self._device_members():
            raise TypeError('Constrained.acq_topk needs device GP members on one device')
        cons = [c._engine() for c in self.constraints]
        obj = None if target is None else self.objective._engine()
        lead = obj if obj is not None else cons[0]
        if isinstance(xgrid, DeviceGrid) and int(xgrid.device) != int(lead.device):
            xgrid = np.asarray(xgrid)                # resident on ANOTHER GPU: through the host, never its pointer
        if not isinstance(xgrid, DeviceGrid):
            xgrid = np.array(xgrid, ndmin=2, dtype=float)
        out = _lib.Engine.constrained_sweep(obj, cons, self.thresholds, 'ei', target, xgrid, k=int(k),
                                            want_all=False)
        self._lead = lead
        return out['top_val'], out['top_idx']

    def acq_batch(self, kind, target, xgrid, nb):
        """nb grid points to evaluate in parallel, on the device (gpx_constrained_sweep_batch): greedy picks of the constrained index
        with target and thresholds frozen and EVERY member -- the objective and each constraint -- conditioned on a pick at its own
        posterior mean (target = None: the probability of feasibility alone, the objective takes no part).  Every member's sweep cache
        is brought onto `xgrid` first (`GP._cache_grid`: a `DeviceGrid` that member's state has swept before is re-used, anything else
        is swept once with the cache on).  Returns dict(sel_val (nb,), sel_idx (nb,), sel_s2 (n, nb)), the objective first.
        Not built: fantasised or pending picks, MCMC / ShardedGP members, off-grid refinement of the picks, pruned seeding of the caches."""
        if kind != 'cei':
            raise ValueError("Constrained.acq_batch takes 'cei', not %r" % (kind,))
        if not self._device_members():
            raise TypeError('Constrained.acq_batch needs device GP members on one device')
        members = self.constraints if target is None else self._members
        if not isinstance(xgrid, DeviceGrid) or int(xgrid.device) != int(members[0].device):
            xgrid = np.array(xgrid, ndmin=2, dtype=float)        # one host copy for all members
        params = ([] if target is None else [float(target)]) + [float(t) for t in self.thresholds]
        kinds = ([] if target is None else ['ei']) + ['pi'] * len(self.constraints)
        engines = [m._cache_grid(k, p, xgrid) for m, k, p in zip(members, kinds, params)]
        obj = None if target is None else engines[0]
        return _lib.Engine.constrained_batch(obj, engines[len(engines) - len(self.constraints):], self.thresholds, 'ei', target, int(nb))

    def topk_engine(self):
        """The device handle whose HBM holds the (value, index) pairs of the last `acq_topk`: the lead of that sweep."""
        lead = getattr(self, '_lead', None)
        return lead if lead is not None else self.objective._engine()
