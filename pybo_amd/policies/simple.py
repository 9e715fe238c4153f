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
carries `index.acq = (kind, param)` and, for models with `acq_batch`, `index.batch(xgrid, nb, **kw)` (pybo_amd/batch.py).
`MES` (max-value entropy search), `KG` (knowledge gradient over a support set), `CEI` (constrained expected improvement on a
`models.Constrained`) and `EHVI` (expected hypervolume improvement on a `models.MultiObjective`) are this build's own: the reference
has none of them.
"""
import numpy as np

__all__ = ['EI', 'PI', 'UCB', 'Thompson', 'MES', 'KG', 'CEI', 'EHVI']


def _attach_topk(index, model, kind, param):
    index.acq = (kind, param)              # the frozen target / beta: what a batch proposal scores every round with
    batch = getattr(model, 'acq_batch', None)
    if batch is not None:                  # device models: nb greedy picks on the swept grid (pybo_amd.propose_batch)
        index.batch = lambda xgrid, nb, **kw: batch(kind, param, xgrid, nb, **kw)
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


def Thompson(model, _, __, n=100, rng=None, method='rff'):
    """Thompson sampling: the index is one posterior function sample built from n random features.  method='pathwise' (device
    models): the feature draw is only the prior, conditioned exactly on the data by the model's factorisation (Matheron's rule)."""
    sample = model.sample_f(n, rng) if method == 'rff' else model.sample_f(n, rng, method=method)
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


def KG(model, bounds, X, nsupport=64, ngrid=10000, support=None, rng=None):
    """Knowledge gradient (Frazier, Powell & Dayanik 2009) over a finite support set A: the expected rise of the maximum posterior
    mean over {x} + A after one noisy observation at x (pybo_amd/kg.py) -- the one policy here that uses the correlation between a
    candidate and the rest of the domain.  Default A: the `nsupport` <= 127 points of `init_uniform(bounds, ngrid, rng)` stacked on X
    with the highest posterior mean (value descending, then index ascending; one `predict_mean`; an ensemble ranks by its
    member-averaged mean).  The model needs `get_knowledge(support, X, grad)` (an ensemble: every member).  The index carries
    `.acq = ('kg', support)` and, for single device GPs, `.topk`; never `.batch` (pybo_amd/batch.py)."""
    from ..inits import init_uniform
    from ..kg import KG_MAX_SUPPORT
    from ..utils import rstate
    if support is None and not 1 <= int(nsupport) <= KG_MAX_SUPPORT:
        raise ValueError('KG: nsupport must be in [1, %d], not %r' % (KG_MAX_SUPPORT, nsupport))
    rng = rstate(rng)
    model = model.copy()
    members = getattr(model, 'members', None)
    lacking = [m for m in ([model] if members is None else [model] + list(members)) if getattr(m, 'get_knowledge', None) is None]
    if lacking:
        raise TypeError('KG needs a model with get_knowledge(support, X, grad); %s has none' % type(lacking[0]).__name__)
    X = np.array(X, ndmin=2, dtype=float)
    if support is None:
        pool = np.vstack([init_uniform(bounds, ngrid, rng), X])
        mean_only = getattr(model, 'predict_mean', None)
        mu = np.asarray(mean_only(pool) if mean_only is not None else model.predict(pool)[0], dtype=float)
        v = np.where(np.isnan(mu), -np.inf, mu)
        support = pool[np.lexsort((np.arange(len(v)), -v))[:int(nsupport)]]
    support = np.array(support, dtype=float).reshape(-1, X.shape[1])
    if not 1 <= len(support) <= KG_MAX_SUPPORT:
        raise ValueError('KG: the support set must have 1 to %d points, not %d' % (KG_MAX_SUPPORT, len(support)))

    def index(X, grad=False):
        return model.get_knowledge(support, X, grad)

    index.acq = ('kg', support)
    fast = getattr(model, 'acq_topk', None) if members is None else None
    if fast is not None:
        index.topk = lambda xgrid, k: fast('kg', support, xgrid, k)
        owner = getattr(model, 'topk_engine', None)
        if owner is not None:
            index.topk_engine = owner
    return index


def CEI(model, _, X, xi=0.0, pmin=0.5):
    """Constrained expected improvement (Gardner et al. 2014; Gelbart et al. 2014) on a `models.Constrained`: EI of the objective
    times the probability that every constraint holds.  The target is the highest objective posterior mean among the observed X
    whose `feasibility` is at least `pmin`, plus xi; while no observation qualifies the index is the probability of feasibility
    alone (target None).  The index carries `.acq = ('cei', target)` and, for models with `acq_topk`, `.topk`; never `.batch`:
    batch proposals (`pybo_amd.propose_batch(..., policy='cei')`, `solve_bayesopt(nbatch=)`) read `.acq` and ask the MODEL -- a
    `models.Constrained` over device members makes its greedy picks in one device call (`acq_batch`: gpx_constrained_sweep_batch),
    any other takes the generic host path, every member believing its own posterior mean at a pick."""
    model = model.copy()
    lacking = [n for n in ('feasibility', 'get_constrained') if getattr(model, n, None) is None]
    if lacking:
        raise TypeError('CEI needs a model with feasibility(X) and get_constrained(target, X, grad); %s has none' % type(model).__name__)
    X = np.array(X, ndmin=2, dtype=float)
    target = None
    if len(X):
        ok = np.asarray(model.feasibility(X)) >= pmin
        if ok.any():
            target = float(np.asarray(model.predict_mean(X))[ok].max() + xi)

    def index(X, grad=False):
        return model.get_constrained(target, X, grad)

    index.acq = ('cei', target)
    fast = getattr(model, 'acq_topk', None)
    if fast is not None and getattr(model, '_device_members', lambda: True)():
        index.topk = lambda xgrid, k: fast('cei', target, xgrid, k)
        owner = getattr(model, 'topk_engine', None)
        if owner is not None:
            index.topk_engine = owner
    return index


def EHVI(model, bounds, X, ref=None):
    """Expected hypervolume improvement (Emmerich et al. 2011) on a `models.MultiObjective`, both objectives maximised.  The front is
    the posterior means of both objectives at the observed X; `ref` (2,) defaults to `F.min(0) - 0.1 span` with span = F.max(0) - F.min(0)
    (1 where that is 0).  The index carries `.acq = ('ehvi', (front, ref))` and, for models with `acq_topk`, `.topk`; never `.batch`."""
    from .. import pareto
    model = model.copy()
    if getattr(model, 'get_ehvi', None) is None:
        raise TypeError('EHVI needs a model with get_ehvi(front, ref, X, grad); %s has none' % type(model).__name__)
    X = np.array(X, ndmin=2, dtype=float)
    front = np.asarray(model.predict_mean(X), dtype=float).reshape(-1, 2) if len(X) else np.empty((0, 2))
    if ref is None:
        ref = pareto.default_ref(front) if len(front) else np.zeros(2)
    ref = np.array(ref, dtype=float).reshape(2)

    def index(X, grad=False):
        return model.get_ehvi(front, ref, X, grad)

    index.acq = ('ehvi', (front, ref))
    fast = getattr(model, 'acq_topk', None)
    if fast is not None and getattr(model, '_device_members', lambda: True)():
        index.topk = lambda xgrid, k: fast('ehvi', (front, ref), xgrid, k)
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
