"""
Acquisition policies EI / PI / UCB / Thompson with pybo's signatures
`policy(model, bounds, X, **kw[, rng]) -> index`, `index(X, grad=False)`
(/root/reference/pybo/policies/simple.py:16-74).  Behaviour kept on purpose:

  * EI / PI copy the model, then take `target = max posterior mean at the observed X + xi`
    (simple.py:20-21, 34-35) -- one `model.predict(X)` per policy call;
  * UCB's `d` is the NUMBER OF OBSERVATIONS len(X), not the input dimension (simple.py:58-60):
    beta = xi*2*log(pi^2/(3 delta)) + xi*(4+N)*log(N+1);
  * Thompson returns ONE posterior function sample's `.get` (simple.py:48); `n` is the number of random
    Fourier features.

New: when the model is the device-backed `pybo_amd.models.GP`, the returned index also carries
`index.topk(xgrid, k)` -- the whole-grid evaluation + top-k done on the GPU in one call -- which
`pybo_amd.solvers.solve_lbfgs` uses instead of `argsort(f(xgrid))` (pybo/solvers/lbfgs.py:50-51).
Any other model (e.g. a test stub) gets plain closures, exactly as in the reference.  Every EI / PI / UCB index also
carries `index.acq = (kind, param)` and, for models with `acq_batch`, `index.batch(xgrid, nb)` (pybo_amd/batch.py).
`MES` (max-value entropy search) is this build's own: the reference has no information-theoretic policy.
"""
import numpy as np

__all__ = ['EI', 'PI', 'UCB', 'Thompson', 'MES']


def _attach_topk(index, model, kind, param):
    index.acq = (kind, param)              # the frozen target / beta: what a batch proposal scores every round with
    batch = getattr(model, 'acq_batch', None)
    if batch is not None:                  # device models: nb greedy picks on the swept grid (pybo_amd.propose_batch)
        index.batch = lambda xgrid, nb: batch(kind, param, xgrid, nb)
    fast = getattr(model, 'acq_topk', None)
    if fast is not None:
        index.topk = lambda xgrid, k: fast(kind, param, xgrid, k)
        owner = getattr(model, 'topk_engine', None)
        if owner is not None:              # which device handle holds the top-k pairs (pybo_amd.dist, comm=)
            index.topk_engine = owner
    return index


def _incumbent_target(model, X, xi):
    """Copy the model (the caller's must stay untouched) and compute best-posterior-mean-at-the-data + xi."""
    snapshot = model.copy()
    mean_only = getattr(snapshot, 'predict_mean', None)      # device models: no variance sweep nobody reads
    mu = mean_only(X) if mean_only is not None else snapshot.predict(X)[0]
    return snapshot, mu.max() + xi


def EI(model, _, X, xi=0.0):
    """Expected improvement over (best posterior mean at the data) + xi."""
    model, target = _incumbent_target(model, X, xi)

    def index(X, grad=False):
        return model.get_improvement(target, X, grad)

    return _attach_topk(index, model, 'ei', target)


def PI(model, _, X, xi=0.05):
    """Probability of improvement over (best posterior mean at the data) + xi."""
    model, target = _incumbent_target(model, X, xi)

    def index(X, grad=False):
        return model.get_tail(target, X, grad)

    return _attach_topk(index, model, 'pi', target)


def Thompson(model, _, __, n=100, rng=None):
    """Thompson sampling: the index is one posterior function sample built from n random features."""
    sample = model.sample_f(n, rng)
    fast = getattr(sample, 'topk', None)
    if fast is None:
        return sample.get

    def index(X, grad=False):
        return sample.get(X, grad)

    index.topk = fast                     # device sample: grid evaluation + top-k stay on the GPU
    return index


def _noise(model):
    """The model's noise variance: its `sn2`, its 'like.sn2' parameter, or 0 for a stub that has neither."""
    sn2 = getattr(model, 'sn2', None)
    if sn2 is None:
        prm = getattr(model, 'params', {}).get('like.sn2')
        sn2 = 0.0 if prm is None else prm.value
    return float(sn2)


def MES(model, bounds, X, nmax=16, ngrid=10000, xi=0.0, rng=None):
    """Max-value entropy search (Wang & Jegelka 2017): mean over nmax sampled maxima y* of g((y* - mu) / s), g(c) = c phi(c) /
    (2 Phi(c)) - log Phi(c) (pybo_amd/mes.py).  The maxima come from the paper's Gumbel approximation on the support set
    `init_uniform(bounds, ngrid, rng)` stacked on X (one `predict` there), floored at (best posterior mean at the data) + xi +
    5 sqrt(sn2).  An ensemble (`models.MCMC`) draws one set per member from that member's own moments: ystar is (n, nmax).
    The index carries `.acq = ('mes', ystar)` and, for device models, `.topk`; never `.batch` (pybo_amd/batch.py)."""
    from ..inits import init_uniform
    from ..mes import mes_value, mes_value_grad, sample_maxima
    from ..utils import rstate
    rng = rstate(rng)
    model = model.copy()
    X = np.array(X, ndmin=2, dtype=float)
    support = np.vstack([init_uniform(bounds, ngrid, rng), X])

    def maxima(member):
        mu, s2 = member.predict(support)
        floor = mu[len(support) - len(X):].max() + xi + 5.0 * np.sqrt(_noise(member))
        return sample_maxima(mu, np.sqrt(s2), nmax, floor, rng)

    members = getattr(model, 'members', None)
    ystar = maxima(model) if members is None else np.array([maxima(m) for m in members])

    if getattr(model, 'get_entropy', None) is not None:
        def index(X, grad=False):
            return model.get_entropy(ystar, X, grad)
    else:
        def index(X, grad=False):
            if not grad:
                return mes_value(*model.predict(X), ystar)
            return mes_value_grad(*model.predict(X, grad=True), ystar)

    index.acq = ('mes', ystar)
    fast = getattr(model, 'acq_topk', None)
    if fast is not None:
        index.topk = lambda xgrid, k: fast('mes', ystar, xgrid, k)
        owner = getattr(model, 'topk_engine', None)
        if owner is not None:
            index.topk_engine = owner
    return index


def UCB(model, _, X, delta=0.1, xi=0.2):
    """GP-UCB.  `delta`: failure probability of the bound; `xi`: scale of the exploration term.
    NB the reference's `d` is len(X), the number of observations (simple.py:58)."""
    model = model.copy()
    nobs = len(X)
    beta = xi * 2 * np.log(np.pi ** 2 / 3 / delta) + xi * (4 + nobs) * np.log(nobs + 1)

    def index(X, grad=False):
        if not grad:
            mu, s2 = model.predict(X)
            return mu + np.sqrt(beta * s2)
        mu, s2, dmu, ds2 = model.predict(X, grad=True)
        width = np.sqrt(beta * s2)
        return mu + width, dmu + 0.5 * np.sqrt(beta / s2[:, None]) * ds2

    return _attach_topk(index, model, 'ucb', beta)
