"""
Recommenders (/root/reference/pybo/recommenders.py:14-35): where to point the user after each step.
`best_latent` maximises the posterior mean starting from the observed points (through solve_lbfgs with
`xgrid=X`), `best_incumbent` returns the observed point with the highest posterior mean.  `best_feasible` (this build's own,
for `models.Constrained`) returns the best observed point that is probably feasible; `best_pareto` (for `models.MultiObjective`) the
observed point whose posterior mean contributes most to the hypervolume.
"""
import numpy as np

from . import solvers

__all__ = ['best_latent', 'best_incumbent', 'best_feasible', 'best_pareto']


def best_latent(model, bounds, X):
    mean_only = getattr(model, 'predict_mean', None)     # device models: no variance, no pass over the factor

    def mean(X, grad=False):
        if mean_only is not None:
            return mean_only(X, grad) if grad else mean_only(X)
        if grad:
            post = model.predict(X, True)
            return post[0], post[2]
        return model.predict(X)[0]

    fast = getattr(model, 'mean_topk', None)        # device models: closed form at the data, else the device sweep
    if fast is not None:
        mean.topk = fast
    xbest, _ = solvers.solve_lbfgs(mean, bounds, xgrid=X)
    return xbest


def best_incumbent(model, _, X):
    mean_only = getattr(model, 'predict_mean', None)
    mu = mean_only(X) if mean_only is not None else model.predict(X)[0]
    return np.asarray(X)[int(np.argmax(mu))]


def best_feasible(model, _, X, pmin=0.5):
    """For a `models.Constrained`: the observed point of highest objective posterior mean among those whose probability of
    feasibility is at least `pmin`; where none qualifies, the observed point of highest feasibility."""
    X = np.array(X, ndmin=2, dtype=float)
    pof = np.asarray(model.feasibility(X), dtype=float)
    ok = pof >= pmin
    if not ok.any():
        return X[int(np.argmax(np.where(np.isnan(pof), -np.inf, pof)))]
    mean_only = getattr(model, 'predict_mean', None)
    mu = np.asarray(mean_only(X) if mean_only is not None else model.predict(X)[0], dtype=float)
    return X[int(np.argmax(np.where(ok & ~np.isnan(mu), mu, -np.inf)))]


def best_pareto(model, _, X, ref=None):
    """For a `models.MultiObjective`: the observed point whose posterior mean (both objectives) has the largest hypervolume
    contribution over `ref` (default: the EHVI policy's, `pareto.default_ref` of the means); ties go to the lowest index.  The whole
    non-dominated set is `model.pareto_set(X)`."""
    from . import pareto
    X = np.array(X, ndmin=2, dtype=float)
    F = np.asarray(model.predict_mean(X), dtype=float).reshape(-1, 2)
    if ref is None:
        ref = pareto.default_ref(F)
    contrib = pareto.hv_contributions(F, ref)
    return X[int(np.argmax(np.where(np.isnan(contrib), -np.inf, contrib)))]
