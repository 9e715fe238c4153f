"""Helper (not a test): problems, handle histories and the reader table of tests/test_gpu_handle_history.py, and the oracle side
of both that file and tests/test_handle_history_cpu.py.

A HISTORY is a way a handle came to hold the first n observations of a problem: fitted from scratch, appended to inside the
padding, grown across a 128-block boundary by the in-place rotation or by re-allocation (grow_block, kernels_grad.hip), refitted
after holding a larger model, grown by an announcement that is never used, or grown by an append that is then refused.  The last
three leave a WHOLE trailing identity block (N <= Np - 128).  A READER is an entry point of the C-ABI; every reader is applied to
every history.

    group R   results depend only on the resident raw data (dXraw, dy, N, Np), the kernel and the call's arguments:
              gpx_loglik_batch, gpx_rff_gram, gpx_rff_gram_batch, gpx_rff_posterior
    group F   results depend on the factor and its inverse (R, T, U, a, alpha): everything else
    group E   the ensemble entry points over members that reached the same data through different histories

Data: synth_problem(400, d, seed=77), length-scales widened by max(1, sqrt(d / 3)) as in tests/test_gpu_warm_queue.py (an appended
point moves nothing otherwise from d ~ 20 on; here it keeps the d = 8 case informative), candidates RandomState(5).rand(300, d).
The oracle objects are computed once per (problem, n) and shared: treat them as read-only."""
import collections
import functools

import numpy as np

from oracle import gp_ref
from helpers import synth_problem

RHO, SN2, BIAS = 1.3, 1e-3, 0.2
PROBLEMS = (('matern5', 3), ('se', 8), ('matern1', 2))
BIG = ('se', 8)                     # the one problem of the 15-block history
N_DATA, N_CAND, N_SEL, SEED = 400, 300, 13001, 77
NB = 128

# tag -> (observations fitted, observations held in the end)
HISTORIES = collections.OrderedDict([
    ('fresh', (120, 120)),                      # control: the table itself is right
    ('pad', (120, 125)),                        # rows written into the padding
    ('restride', (120, 131)),                   # in-place rotation (grow_block, first branch); capacity unchanged
    ('realloc', (120, 260)),                    # 128 by rotation, 256 by re-allocation, then 4 more rows; capacity grew
    ('reused', (120, 131)),                     # after a 400-point model of another kernel and hypers: stale head-room
    ('announced_unused', (128, 128)),           # cached sweep, append_begin at N == Np, nothing else: trailing empty block
    ('announced_then_other', (128, 129)),       # ... then a DIFFERENT point appended: a plain append into the grown block
    ('refused_at_boundary', (128, 128)),        # append of a point with a NaN coordinate at N == Np: grown, then refused
    ('big_trailing_block', (1920, 1920)),       # 15 blocks, cached sweep, append_begin: an empty 16th block (nP = 16)
])
# the handle's padded size Np after the history
NP_AFTER = dict(fresh=128, pad=128, restride=256, realloc=384, reused=256, announced_unused=256, announced_then_other=256,
                refused_at_boundary=256, big_trailing_block=2048)
SEL_G = 4096                        # candidates of one generation of a selection-only sweep at these sizes (prune_geom, api.hip)
SURVIVOR_KS = (10, 32, 64, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048)
# the handle's padded size equals a fresh fit's on the same data: group R must give the fresh fit's BITS there
SAME_NP = ('fresh', 'pad', 'restride', 'realloc', 'reused', 'announced_then_other')
TRAILING_EMPTY = ('announced_unused', 'refused_at_boundary', 'big_trailing_block')
# the earlier tenant of the 'reused' handle: same d, another kernel, other hyper-parameters, 400 observations of another draw
OTHER = dict(kernel={'matern5': 'se', 'se': 'matern3', 'matern1': 'matern5'}, rho=0.7, sn2=5e-3, bias=-0.4, seed=78)
# members of the ensemble (group E): (sn2, rho, factor on ell, bias)
ENS_HYPERS = ((SN2, RHO, 1.0, BIAS), (5e-3, 1.6, 1.4, 0.3), (2e-4, 0.7, 0.7, -0.1))
ENS_N = 131


def acqs(target):
    """(acquisition, parameter) of the cold sweeps, as tests/test_gpu_parity.py::test_acquisition_values_and_topk: `target` is the
    oracle's largest posterior mean at the observations."""
    return (('ei', target + 0.01), ('pi', target + 0.01), ('ucb', 3.7), ('mean', None))


def ens_acqs(target):
    return (('ei', target), ('ucb', 3.0))


def ens_ref(refs, kind, param, Z):
    """(values, mixture mean, mixture variance) of the oracle members' average, as tests/test_gpu_ensemble_grid.py forms it."""
    post = [r.predict(Z) for r in refs]
    mus, s2s = np.array([p[0] for p in post]), np.array([p[1] for p in post])
    mu = mus.mean(0)
    s2 = np.maximum((s2s + mus ** 2).mean(0) - mu ** 2, 0.0)
    if kind == 'ei':
        return np.mean([r.get_improvement(param, Z) for r in refs], axis=0), mu, s2
    return mu + np.sqrt(param * s2), mu, s2


def cells():
    """(history, kernel, d) of every cell of the matrix."""
    out = []
    for tag in HISTORIES:
        for kernel, d in PROBLEMS:
            if tag == 'big_trailing_block' and (kernel, d) != BIG:
                continue
            out.append((tag, kernel, d))
    return out


class Problem(object):
    """Data, hyper-parameters and candidates of one problem; observation i is (X[i], y[i]), a model holds the first n of them."""

    def __init__(self, kernel, d, ndata=N_DATA):
        self.kernel, self.d = kernel, d
        self.kid = gp_ref.KERNEL_IDS[kernel]
        self.X, self.y, ell = synth_problem(ndata, d, seed=SEED)
        self.ell = ell * max(1.0, np.sqrt(d / 3.0))
        self.Zp = np.random.RandomState(5).rand(N_CAND, d)
        # the selection-only sweep prunes from 3 generations of 4096 candidates on (prune_geom, api.hip): 13001 is off every tile
        self.Zsel = np.random.RandomState(6).rand(N_SEL, d)
        for a in (self.X, self.y, self.ell, self.Zp, self.Zsel):
            a.setflags(write=False)
        self._ref = {}
        self._raw = {}

    def make_ref(self, X, y, hyp=None):
        sn2, rho, fell, bias = (SN2, RHO, 1.0, BIAS) if hyp is None else hyp
        r = gp_ref.make_gp(sn2, rho, self.ell * fell, bias, self.kernel)
        r.add_data(X, y)
        return r

    def ref(self, n):
        """(oracle fitted on the first n observations, its mu and s2 over Zp): computed once per n."""
        if n not in self._ref:
            r = self.make_ref(self.X[:n], self.y[:n])
            mu, s2 = r.predict(self.Zp)
            mu.setflags(write=False)
            s2.setflags(write=False)
            self._ref[n] = (r, mu, s2)
        return self._ref[n]

    def phantom(self, n):
        """The oracle on the first n observations PLUS one phantom observation (x = 0, y = 0): what a padded row looks like when
        it is read as data."""
        return self.make_ref(np.vstack([self.X[:n], np.zeros((1, self.d))]), np.hstack([self.y[:n], 0.0]))

    def greedy(self, n, nb=4):
        """(target, tests/batch_ref.py's from-scratch greedy EI batch of nb picks over Zp) on the first n observations."""
        if ('greedy', n) not in self._ref:
            import batch_ref
            target = float(self.ref(n)[0].mean_at_obs().max())
            self._ref[('greedy', n)] = (target, batch_ref.greedy(self.X[:n], self.y[:n], self.Zp, self.kernel, self.ell, RHO, SN2,
                                                                 BIAS, 'ei', target, nb))
        return self._ref[('greedy', n)]

    def survivor_k(self, n):
        """(k, survivors the oracle predicts) for a pruned selection-only EI sweep of Zsel that has SURVIVORS: with k = 10 the 4096
        seeds (largest bound EI(mu, sqrt(rho))) hold the whole top-k and every other bound is below tau, so the survivor pass and
        the second bound never run.  tau falls as k grows; the first k of SURVIVOR_KS whose predicted count of unevaluated
        candidates with a bound >= tau (the k-th best seed value) lies in [50, 3000] is taken -- away from 0 and from the cap of
        4096 (max(G, M / 4), prune_geom) by far more than the bound's delta ~ 1e-12 can move.  None: no such k."""
        if ('surv', n) not in self._ref:
            import batch_ref
            r = self.ref(n)[0]
            target = acqs(float(r.mean_at_obs().max()))[0][1]
            mu, s2 = r.predict(self.Zsel)
            ei = batch_ref.acq_from_moments('ei', target, mu, s2)
            ub = batch_ref.acq_from_moments('ei', target, mu, np.full_like(mu, RHO))
            seeds = np.argsort(-ub, kind='stable')[:SEL_G]
            rest = np.ones(len(mu), dtype=bool)
            rest[seeds] = False
            best = np.sort(ei[seeds])[::-1]
            found = None
            for k in SURVIVOR_KS:
                nsurv = int(np.sum(ub[rest] >= best[k - 1]))
                if 50 <= nsurv <= 3000:
                    found = (k, nsurv)
                    break
            self._ref[('surv', n)] = found
        return self._ref[('surv', n)]

    # ---- group R: the calls' arguments and the oracle's answers ----------------------------------------------------------------
    def raw_args(self):
        """The arguments of the group-R readers (the same for every history of the problem)."""
        if 'args' not in self._raw:
            d = self.d
            th0 = np.concatenate([[np.log(SN2), np.log(RHO)], np.log(self.ell), [BIAS]])
            thetas = th0 + 0.4 * np.random.RandomState(94).randn(9, d + 3)          # as tests/test_gpu_mcmc.py
            hyp = np.column_stack([np.exp(thetas[:, :2 + d]), thetas[:, 2 + d]])
            draws = {}
            for n in (30, 130):                 # n >= 128 takes the per-draw path of the feature Gram
                W, b, z = [], [], []
                for s in range(3):
                    rng = np.random.RandomState(100 * n + s)
                    Ws, bs = gp_ref.rff_draw_spectral(self.kid, n, d, self.ell, rng)
                    W.append(Ws), b.append(bs), z.append(rng.randn(n))
                draws[n] = (np.array(W), np.array(b), np.array(z))
            self._raw['args'] = dict(thetas=thetas, hyp=hyp, draws=draws)
        return self._raw['args']

    def raw_ref(self, n):
        """The oracle's answers to the group-R readers on the first n observations, keyed like read_raw's."""
        if n not in self._raw:
            args = self.raw_args()
            X, y = self.X[:n], self.y[:n]
            r = self.make_ref(X, y)
            ll = []
            for th in args['thetas']:
                r.set_hyper_vector(th)
                ll.append(r.loglikelihood())
            out = collections.OrderedDict(loglik_batch=np.array(ll))
            for n_f, (W, b, z) in args['draws'].items():
                A, v, th = [], [], []
                for s in range(len(W)):
                    C = np.cos(X @ W[s].T + b[s])
                    A.append(C.T @ C), v.append(C.T @ (y - BIAS))
                    th.append(gp_ref.rff_posterior_theta(A[-1], v[-1], n_f, RHO, SN2, z[s]))
                out['rff_gram_A_%d' % n_f], out['rff_gram_v_%d' % n_f] = A[0], v[0]
                if n_f == 30:
                    out['rff_gram_batch_A'], out['rff_gram_batch_v'] = np.array(A), np.array(v)
                out['rff_posterior_%d' % n_f] = np.array(th)
            self._raw[n] = out
        return self._raw[n]


@functools.lru_cache(maxsize=None)
def problem(kernel, d, big=False):
    return Problem(kernel, d, 1923 if big else N_DATA)


def problem_of(tag, kernel, d):
    return problem(kernel, d, tag == 'big_trailing_block')


def read_raw(e, P):
    """Every group-R reader on handle `e`: an ordered dict of arrays, keyed like Problem.raw_ref's."""
    args = P.raw_args()
    out = collections.OrderedDict(loglik_batch=e.loglik_batch(args['hyp']))
    for n_f, (W, b, z) in args['draws'].items():
        out['rff_gram_A_%d' % n_f], out['rff_gram_v_%d' % n_f] = e.rff_gram(W[0], b[0])
        if n_f == 30:
            out['rff_gram_batch_A'], out['rff_gram_batch_v'] = e.rff_gram_batch(W, b)
        out['rff_posterior_%d' % n_f] = e.rff_posterior(W, b, z, np.sqrt(2.0 * RHO / n_f))
    return out


def raw_tol(key, want):
    """(rtol, atol) of a group-R output against the oracle: gpx_loglik_batch's of tests/test_gpu_mcmc.py, the feature Gram's and the
    weight posterior's of tests/test_gpu_parity.py::test_rff_paths_match_oracle."""
    if key == 'loglik_batch':
        return 1e-9, 0.0
    if key.startswith('rff_posterior'):
        return 0.0, 1e-7 * np.abs(want).max(axis=-1, keepdims=True)
    return 1e-11, 1e-10


# ---- histories on the device ------------------------------------------------------------------------------------------------------
def make_cache(e, Z):
    e.set_option('sweep_cache', 1)
    e.sweep('ei', 0.5, Z, k=0, want_all=False)
    e.set_option('sweep_cache', 0)
    assert e.sweep_cache_size() == len(Z)


def twin(P, n, hyp=None):
    """A fresh handle fitted from scratch on the first n observations."""
    from pybo_amd._lib import Engine
    sn2, rho, fell, bias = (SN2, RHO, 1.0, BIAS) if hyp is None else hyp
    e = Engine(0)
    e.fit(P.X[:n], P.y[:n], P.kernel, P.ell * fell, rho, sn2, bias)
    return e


def build(tag, P, hyp=None, upto=None):
    """(handle, n): a handle that reached the first n observations of P through history `tag`; every state the history is about is
    asserted here.  `upto`: append the following observations as well (group E brings its members to the same data)."""
    from pybo_amd._lib import Engine
    n_fit, n_end = HISTORIES[tag]
    sn2, rho, fell, bias = (SN2, RHO, 1.0, BIAS) if hyp is None else hyp
    e = Engine(0)
    if tag == 'reused':
        Xo, yo, ello = synth_problem(N_DATA, P.d, seed=OTHER['seed'])
        e.fit(Xo, yo, OTHER['kernel'][P.kernel], ello, OTHER['rho'], OTHER['sn2'], OTHER['bias'])
        e.predict(P.Zp[:5])                     # the larger model's inverse, solve vectors and scratch exist too
        assert e.capacity() >= 512
    e.fit(P.X[:n_fit], P.y[:n_fit], P.kernel, P.ell * fell, rho, sn2, bias)
    cap0 = e.capacity()
    n = n_fit
    if tag in ('announced_unused', 'announced_then_other', 'big_trailing_block'):
        assert n_fit % NB == 0
        make_cache(e, P.Zp)
        assert e.append_begin(P.X[n_fit + 2])   # grows the factor (N == Np); this point is never the next one appended
        assert e.N == n_fit and e.capacity() == cap0
    if tag == 'refused_at_boundary':
        x = np.array(P.X[n_fit])
        x[0] = np.nan                           # k(X, x) = NaN -> d^2 = NaN: refused by k_append_dots AFTER the factor has grown
        try:
            e.append(x, P.y[n_fit])
        except np.linalg.LinAlgError:
            pass
        else:
            raise AssertionError('an observation with a NaN coordinate was accepted')
        assert e.N == n_fit and e.fail_pivot() == n_fit and e.sweep_cache_size() == 0 and e.capacity() == cap0
    for i in range(n_fit, n_end if upto is None else upto):
        assert e.append(P.X[i], P.y[i])
        n += 1
    assert e.N == n
    if upto is None:
        if tag in ('restride', 'reused', 'announced_then_other'):
            assert e.capacity() == cap0 and n > -(-n_fit // NB) * NB          # past the fit's last block, no allocation
        if tag == 'realloc':
            assert e.capacity() > cap0
        if tag == 'pad':
            assert e.capacity() == cap0
    return e, n
