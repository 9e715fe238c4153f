"""
Point estimate of the hyper-parameters: maximise the density the sampler of `mcmc.py` draws from,

    log p(y | theta) + log prior(theta) + log-Jacobian,      theta = [log sn2, log rho, log ell_1..d, bias]

(ML-II when no priors are recorded, MAP otherwise) with L-BFGS-B on the analytic gradient.  One evaluation is one fit
plus `loglikelihood(grad=True)` -- for the device model `gpx_loglik_grad`, one triangular product instead of the d + 3
extra factorisations finite differences of `loglik_at` cost.  Host logic only: works with ANY model offering
`hyper_vector() / set_hyper_vector(theta) / loglikelihood(grad=True) / params`, which is how the CPU tests drive it
with the oracle model.
"""
import numpy as np
from scipy.optimize import fmin_l_bfgs_b

from .mcmc import _log_prior_part
from .priors import log_prior_grad, prior_bounds

__all__ = ['optimize', 'log_target_grad', 'target_bounds']

_REFUSED = 1e25         # what a state without a density (not positive definite, outside a support) costs the line search
_NAMES = ('like.sn2', 'kern.rho', 'kern.ell', 'mean.bias')


def target_bounds(model):
    """(lo, hi) of the box in theta: the uniform priors' support intersected with |theta| <= 60 (the sampler's own limit
    on the log-parameters; the bias is bounded by its prior alone)."""
    d = len(model.hyper_vector()) - 3
    sizes = (1, 1, d, 1)
    lo, hi = [], []
    for name, n in zip(_NAMES, sizes):
        a, b = prior_bounds(model.params[name].prior, n)
        if name != 'mean.bias':
            with np.errstate(divide='ignore'):
                a, b = np.log(np.maximum(a, 0.0)), np.log(b)
            a, b = np.maximum(a, -60.0), np.minimum(b, 60.0)
        lo.append(a)
        hi.append(b)
    return np.concatenate(lo), np.concatenate(hi)


def log_target_grad(model, theta):
    """(value, gradient) of the target at `theta`; the model is left fitted there.  (-inf, zeros) where the target has
    no density."""
    theta = np.asarray(theta, dtype=float)
    d = len(theta) - 3
    lp = _log_prior_part(model, theta)
    if not np.isfinite(lp):
        return -np.inf, np.zeros(len(theta))
    try:
        model.set_hyper_vector(theta)
        L, g = model.loglikelihood(grad=True)
    except np.linalg.LinAlgError:
        return -np.inf, np.zeros(len(theta))
    if not np.isfinite(L):
        return -np.inf, np.zeros(len(theta))
    x = np.concatenate([np.exp(theta[:2 + d]), theta[2 + d:]])
    pr = model.params
    gp = np.concatenate([np.atleast_1d(log_prior_grad(pr['like.sn2'].prior, x[0])),
                         np.atleast_1d(log_prior_grad(pr['kern.rho'].prior, x[1])),
                         np.atleast_1d(log_prior_grad(pr['kern.ell'].prior, x[2:2 + d])),
                         np.atleast_1d(log_prior_grad(pr['mean.bias'].prior, x[2 + d]))])
    gp[:2 + d] = gp[:2 + d] * x[:2 + d] + 1.0          # chain rule of x = exp(theta), and the Jacobian's own derivative
    return float(lp + L), np.asarray(g, dtype=float) + gp


def optimize(model, maxiter=200, rng=None, pgtol=1e-5, factr=1e7, info=None):
    """Set `model`'s hyper-parameters to the best state L-BFGS-B sees from the current one and return the model.
    `rng` is accepted for symmetry with `MCMC` (the search is deterministic and draws nothing).  `info`: a dict that
    receives {'theta', 'target', 'start_target', 'nfev', 'warnflag', 'bounds'}."""
    theta0 = np.array(model.hyper_vector(), dtype=float)
    lo, hi = target_bounds(model)
    best = {'f': -np.inf, 'theta': theta0.copy()}
    nfev = [0]

    def neg(theta):
        nfev[0] += 1
        f, g = log_target_grad(model, theta)
        if not np.isfinite(f):
            return _REFUSED, np.zeros(len(theta))       # large and flat: the line search backs off
        if f > best['f']:
            best['f'], best['theta'] = f, np.array(theta, dtype=float)
        return -f, -g

    start = -neg(theta0)[0]
    if start == -_REFUSED:
        raise ValueError('optimize: the initial hyper-parameters have zero posterior density')
    bounds = [(None if not np.isfinite(a) else a, None if not np.isfinite(b) else b) for a, b in zip(lo, hi)]
    _, _, res = fmin_l_bfgs_b(neg, np.clip(theta0, lo, hi), bounds=bounds, maxiter=int(maxiter), pgtol=pgtol, factr=factr)
    model.set_hyper_vector(best['theta'])
    if info is not None:
        info.update(theta=best['theta'].copy(), target=best['f'], start_target=start, nfev=nfev[0],
                    warnflag=res['warnflag'], bounds=(lo, hi))
    return model
