"""Every entry point of the C-ABI on handles that were appended to, grown, reused or announced to: the history x reader matrix of
tests/history_ref.py.  Almost every other comparison of the suite runs on a handle straight after gpx_fit; in the product (the BO
loop, the MCMC sampler's pooled handles) a handle is almost never in that state, and three histories leave one no other test
enters: a whole trailing identity block (N <= Np - 128).

One test per (history, problem, reader group); each builds its own instance of the history, which asserts that it entered its state
(capacity, N, fail pivot, cache size: history_ref.build).

    raw      group R first, straight after the history: gpx_loglik_batch (9 vectors), gpx_rff_gram (n = 30, 130), gpx_rff_gram_batch
             (S = 3, n = 30), gpx_rff_posterior (n = 30, 130).  Against the oracle at their own tests' tolerances; and where the handle's
             padded size is a fresh fit's (history_ref.SAME_NP) array-equal to a fresh twin -- a reader that does not repeat its own
             bits on the twin would be held to the oracle's tolerance only (each output prints which it was).  With another padded
             size the summation may be partitioned differently: oracle tolerance, and whether the bits were equal is printed.
             On the MI355X every reader repeated its bits on the twin, and the only output whose bits differed from the twin's was
             gpx_loglik_batch on big_trailing_block (16 block rows against the twin's 15, the task-graph path; both 3e-13 from the oracle).
    factor   group F: loglik, loglik_grad, mean_at_obs, var_at_obs, get_matrix, get_vectors, predict with both gradient forms,
             predict_mean, predict_cov, sample_joint, cold sweeps (EI, PI, UCB, mean), the selection-only sweep, MES, and a cache
             made afterwards with sweep_batch on it -- each against the oracle at the tolerance its own test uses.  The
             selection-only sweep runs over the 300 candidates as well as over 13001: below 12288 candidates prune = 1 takes the
             plain loop, and with k = 10 the pruned sweep has no survivors; so it also runs at a k for which the oracle predicts
             some (history_ref.Problem.survivor_k; the device's count equalled the oracle's in every cell), with the second bound on.
    ensemble group E: members that reached the same 131 observations by 120 + 11 appends across the rotation (the lead), by 128 + an
             unused announcement + 3 appends, and by a fresh fit; against three fresh twins and the oracle's member average.

After the readers predict(Zp) runs once more: array-equal to the first one of this instance and to the other group's instance (no
reader disturbed the model).  A reader that misses its check does not stop the others: the failures are gathered per cell.

The conditions that make these comparisons sharp are asserted on the CPU, tests/test_handle_history_cpu.py."""
import numpy as np
import pytest

import batch_ref
import history_ref as H
import hyper_ref
import joint_ref
import mes_ref
from history_ref import RHO, SN2
from oracle import gp_ref
from helpers import s2_tol, mu_tol, ei_tol

pytestmark = pytest.mark.gpu

CELLS = H.cells()
JIT = 1e-10 * RHO
EPS = 2.0 ** -52
_PREDICT = {}               # (history, kernel) -> predict(Zp) of the instance that ran first


class Checks(object):
    """Gathers a cell's failed checks so that one run names them all."""

    def __init__(self, cell):
        self.cell, self.failed = cell, []

    def __call__(self, name, ok, detail=''):
        if not bool(ok):
            self.failed.append('%s %s' % (name, detail))
            print('FAILED', self.cell, name, detail)

    def within(self, name, got, want, tol):
        err = np.abs(np.asarray(got) - np.asarray(want))
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = float(np.nanmax(np.where(err > 0, err / tol, 0.0))) if err.size else 0.0
        print('%-28s err / tol %.3g' % (name, ratio))
        self(name, np.all(err <= tol) and np.all(np.isfinite(got)), 'worst err / tol %.3g' % ratio)

    def done(self):
        assert not self.failed, (self.cell, self.failed)


def _model_is_undisturbed(ck, e, P, n, key, first=None):
    _, mr, sr = P.ref(n)
    mu, s2 = e.predict(P.Zp)
    ck.within('predict(Zp) mu', mu, mr, mu_tol(mr, RHO))
    ck.within('predict(Zp) s2', s2, sr, s2_tol(sr, RHO))
    if first is not None:
        ck('predict(Zp) after the readers', np.array_equal(mu, first[0]) and np.array_equal(s2, first[1]), 'bits moved')
    other = _PREDICT.setdefault(key, (mu, s2))
    ck('predict(Zp) on the other instance', np.array_equal(mu, other[0]) and np.array_equal(s2, other[1]), 'bits differ')
    return mu, s2


# ---------------------------------------------------------------------------------------------------------------------------------
# group R
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,kernel,d', CELLS)
def test_raw(tag, kernel, d):
    P = H.problem_of(tag, kernel, d)
    ck = Checks((tag, kernel, 'raw'))
    e, n = H.build(tag, P)
    got = H.read_raw(e, P)                      # the first calls after the history
    want = P.raw_ref(n)
    t = H.twin(P, n)
    twin_a, twin_b = H.read_raw(t, P), H.read_raw(t, P)
    t.close()
    for key in got:
        rtol, atol = H.raw_tol(key, want[key])
        tol = atol + rtol * np.abs(want[key])
        ck.within(key, got[key], want[key], tol)
        ck.within(key + ' (twin)', twin_a[key], want[key], tol)
        repeats, same = np.array_equal(twin_a[key], twin_b[key]), np.array_equal(got[key], twin_a[key])
        print('%-28s twin repeats its bits: %s; handle == twin bit for bit: %s' % (key, repeats, same))
        if tag in H.SAME_NP and repeats:
            ck(key + ' == twin', same, 'max |diff| %.3g' % np.abs(got[key] - twin_a[key]).max())
    again = H.read_raw(e, P)
    for key in got:
        if np.array_equal(twin_a[key], twin_b[key]):
            ck(key + ' repeats', np.array_equal(again[key], got[key]))
    _model_is_undisturbed(ck, e, P, n, (tag, kernel))
    e.close()
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# group F
# ---------------------------------------------------------------------------------------------------------------------------------
def _moments_and_matrices(ck, e, P, n):
    ref = P.ref(n)[0]
    X = P.X[:n]
    ll = ref.loglikelihood()
    ck.within('loglik', e.loglik(), ll, 1e-9 * abs(ll))
    want, S = hyper_ref.loglik_grad(ref)
    L, g = e.loglik_grad()
    ck('loglik_grad value', L == e.loglik())
    ck.within('loglik_grad', g, want, 1e-6 * S)
    mo, so = ref.predict(X)
    mu, mx = e.mean_at_obs()
    ck.within('mean_at_obs', mu, mo, 1e-8)
    ck('mean_at_obs max', mx == mu.max())
    ck.within('var_at_obs', e.var_at_obs(), so, s2_tol(so, RHO))
    Lf, T, K = e.get_matrix('L'), e.get_matrix('T'), ref.gram()
    ck('L, T lower triangular', np.array_equal(Lf, np.tril(Lf)) and np.array_equal(T, np.tril(T)))
    ck.within('|L L^T - K| / |K|', np.linalg.norm(Lf @ Lf.T - K) / np.linalg.norm(K), 0.0, 1e-13)
    ck.within('max |T L - I|', np.max(np.abs(T @ Lf - np.eye(n))), 0.0, 1e-9)
    a, alpha = e.get_vectors()                  # (tests/test_gpu_parity.py::test_fit_stages_match_oracle)
    ck.within('a', a, ref.a, 1e-9 * np.abs(ref.a).max())
    ck.within('alpha', alpha, ref.alpha(), 1e-8 * np.abs(ref.alpha()).max())


def _point_predictions(ck, e, P, n):
    ref = P.ref(n)[0]
    Z = P.Zp[:19]
    want = ref.predict(Z, grad=True)
    grads = P.kernel != 'matern1'               # (the exponential kernel's kink: skipped as tests/test_gpu_fuzz.py does)

    def gtol(w):
        return 1e-8 + 1e-6 * np.abs(w)
    for form, Zf in ((1, Z), (2, Z), (0, Z[:1])):
        e.set_option('grad_form', form)
        got = e.predict(Zf, grad=True)
        m = len(Zf)
        ck.within('predict form %d mu' % form, got[0], want[0][:m], mu_tol(want[0][:m], RHO))
        ck.within('predict form %d s2' % form, got[1], want[1][:m], s2_tol(want[1][:m], RHO))
        if grads:
            ck.within('predict form %d dmu' % form, got[2], want[2][:m], gtol(want[2][:m]))
            ck.within('predict form %d ds2' % form, got[3], want[3][:m], gtol(want[3][:m]))
    e.set_option('grad_form', 0)
    m1, dm1 = e.predict_mean(Z, grad=True)
    ck.within('predict_mean', m1, want[0], mu_tol(want[0], RHO))
    if grads:
        ck.within('predict_mean gradient', dm1, want[2], gtol(want[2]))
    # the joint posterior (tests/test_gpu_joint.py): two panels, the second ragged
    Zj = P.Zp[:130]
    M = len(Zj)
    mj, Sigma = joint_ref.joint(ref, Zj)
    mu, cov = e.predict_cov(Zj)
    ck.within('predict_cov mu', mu, mj, mu_tol(mj, RHO))
    ck.within('predict_cov', cov, Sigma, joint_ref.cov_tol(Sigma, RHO))
    ck('predict_cov symmetric', np.array_equal(cov, cov.T))
    R = None
    for noisy in (False, True):
        D = e.sample_joint(Zj, np.eye(M), noisy=noisy, jitter=JIT) - mu[None, :]
        A = cov + (JIT + (SN2 if noisy else 0.0)) * np.eye(M)
        ck('sample_joint factor upper triangular', np.array_equal(D, np.triu(D)))
        ck.within('sample_joint factor residual (noisy %d)' % noisy, np.linalg.norm(D.T @ D - A) / np.linalg.norm(A), 0.0, 1e-13)
        R = D if not noisy else R
    # draws against mu + z R with R read through z = 2^40 I and an M-term dot product's rounding (test_gpu_joint.py, item 7)
    Rx = (e.sample_joint(Zj, 2.0 ** 40 * np.eye(M), jitter=JIT) - mu[None, :]) * 2.0 ** -40
    ck('sample_joint factor read twice', np.all(np.abs(Rx - R) <= 2.0 * EPS * (np.abs(mu)[None, :] + np.abs(R))))
    z = np.random.RandomState(7).randn(3, M)
    out = e.sample_joint(Zj, z, jitter=JIT)
    wantd = mu[None, :].astype(np.longdouble) + z.astype(np.longdouble) @ Rx.astype(np.longdouble)
    bound = (M + 2) * EPS * (np.abs(z) @ np.abs(Rx)) + EPS * np.abs(mu)[None, :]
    ck.within('sample_joint draws', out, np.asarray(wantd, dtype=float), bound)


def _selection_only(ck, e, P, n, nP, target):
    """The selection-only call (k = 10, no other output) with prune = 1 against prune = 0 on the same handle, over the 300 candidates
    (too few to prune: the plain loop under both) and over 13001, where prune = 1 runs the bound pass, the seeds and the survivors --
    once with the first bound alone and once with the second bound over min(2, nP, N / 128) leading block rows."""
    small = {}
    for p in (1, 0):
        e.set_option('prune', p)
        small[p] = e.sweep('ei', target, P.Zp, k=10, want_all=False)
    ck('selection-only over Zp: prune = 1 == prune = 0', np.array_equal(small[1]['top_idx'], small[0]['top_idx']) and
       np.array_equal(small[1]['top_val'], small[0]['top_val']))
    e.set_option('prune', -1)
    full = e.sweep('ei', target, P.Zsel, k=10)
    order = gp_ref.topk_desc(full['acq'], 10)
    ck('sweep over Zsel top-k ranks its own values', np.array_equal(full['top_idx'], order))
    for prune, rows in ((0, -1), (1, 0), (1, 2)):
        e.set_option('prune', prune)
        e.set_option('prune_rows', rows)
        r = e.sweep('ei', target, P.Zsel, k=10, want_all=False)
        rep = e.prune_report(vectors=False)
        print('selection-only prune %d rows %d: %s, %d survivors, nR %d, %d after the second bound' % (
            prune, rows, rep['path'], rep['nsurv'], rep['nR'], rep['nsurv2']))
        name = 'selection-only over Zsel (prune %d, prune_rows %d)' % (prune, rows)
        ck(name, np.array_equal(r['top_idx'], order) and np.array_equal(r['top_val'], full['acq'][order]), (r['top_idx'], order))
        # (prune = 1: the bound pass and the seeds ran; 'fell back' where more than a quarter survived -- a dense model's flat bound)
        ck(name + ' path', rep['path'] == 'plain' if prune == 0 else rep['path'] in ('pruned', 'fell back'), rep['path'])
        ck(name + ' prefix rows hold data only', rep['nR'] <= n // H.NB, rep['nR'])
    # ... and at the k the oracle predicts survivors for (Problem.survivor_k): their exact pass and the second bound's cut run too
    k2, predicted = P.survivor_k(n)
    r = e.sweep('ei', target, P.Zsel, k=k2, want_all=False)
    rep = e.prune_report(vectors=False)
    print('selection-only k = %d: %s, %d survivors (oracle: %d), nR %d, %d after the second bound' % (
        k2, rep['path'], rep['nsurv'], predicted, rep['nR'], rep['nsurv2']))
    order = gp_ref.topk_desc(full['acq'], k2)
    ck('selection-only with survivors', np.array_equal(r['top_idx'], order) and np.array_equal(r['top_val'], full['acq'][order]))
    ck('selection-only with survivors path', rep['path'] == 'pruned' and rep['nsurv'] > 0, (rep['path'], rep['nsurv']))
    ck('second bound over whole data blocks', rep['nR'] == min(2, nP, n // H.NB), (rep['nR'], nP, n))
    e.set_option('prune', -1)
    e.set_option('prune_rows', -1)


def _sweeps(ck, e, P, n, nP):
    ref, mr, sr = P.ref(n)
    Zp = P.Zp
    target, greedy = P.greedy(n)
    mean_bits = None
    for kind, param in H.acqs(target):          # tests/test_gpu_parity.py::test_acquisition_values_and_topk
        want = mr if kind == 'mean' else batch_ref.acq_from_moments(kind, param, mr, sr)
        r = e.sweep(kind, param, Zp, k=10, want_moments=True)
        got = r['acq']
        big = np.abs(want) > 1e-12 * np.abs(want).max()
        ck.within('sweep %s values' % kind, got[big], want[big], 1e-6 * np.abs(want[big]))
        ck.within('sweep %s mu' % kind, r['mu'], mr, mu_tol(mr, RHO))
        ck.within('sweep %s s2' % kind, r['s2'], sr, s2_tol(sr, RHO))
        ck('sweep %s top-k ranks its own values' % kind,np.array_equal(r['top_idx'], gp_ref.topk_desc(got, 10)) and
           np.array_equal(r['top_val'], got[r['top_idx']]))
        ck('sweep %s winner' % kind, r['top_idx'][0] == int(np.argmax(want)), (r['top_idx'][0], int(np.argmax(want))))
        if kind == 'ei':
            _selection_only(ck, e, P, n, nP, param)
        if kind == 'mean':
            mean_bits = (r['mu'], r['s2'])
    # max-value entropy search (tests/test_gpu_mes.py): the 'mean' sweep's moments bit for bit, the value within the derived bound
    ys = target + 0.05 + 0.8 * np.random.RandomState(13).rand(7)
    r = e.sweep('mes', ys, Zp, k=10, want_moments=True)
    ck('mes moments', np.array_equal(r['mu'], mean_bits[0]) and np.array_equal(r['s2'], mean_bits[1]))
    rows = np.arange(0, len(Zp), 15)
    bad, worst = mes_ref.check_mes(r['mu'][rows], r['s2'][rows], ys, r['acq'][rows])
    print('%-28s err / tol %.3g' % ('mes values', worst))
    ck('mes values', not bad.any(), (worst, rows[bad][:5]))
    ck('mes top-k', np.array_equal(r['top_idx'], gp_ref.topk_desc(r['acq'], 10)))
    # a cache made now, and four greedy picks on it (tests/test_gpu_batch.py)
    H.make_cache(e, Zp)
    got = e.sweep_batch('ei', target, 4)
    ck('sweep_batch margins admit the case', greedy['margin'].min() >= batch_ref.MIN_MARGIN)
    ck('sweep_batch picks', np.array_equal(got['sel_idx'], greedy['idx']), (got['sel_idx'], greedy['idx']))
    ck.within('sweep_batch s2', got['sel_s2'], greedy['s2'], s2_tol(greedy['s2'], RHO))
    ck.within('sweep_batch values', got['sel_val'], greedy['val'], ei_tol(greedy['mu_pick'], greedy['s2'], target, RHO))
    warm = e.sweep_update('ei', target, k=1, want_moments=True)
    ck.within('re-score of the new cache mu', warm['mu'], mr, mu_tol(mr, RHO))
    ck.within('re-score of the new cache s2', warm['s2'], sr, s2_tol(sr, RHO))


@pytest.mark.parametrize('tag,kernel,d', CELLS)
def test_factor(tag, kernel, d):
    P = H.problem_of(tag, kernel, d)
    ck = Checks((tag, kernel, 'factor'))
    e, n = H.build(tag, P)
    first = _model_is_undisturbed(ck, e, P, n, (tag, kernel))
    _moments_and_matrices(ck, e, P, n)
    _point_predictions(ck, e, P, n)
    _sweeps(ck, e, P, n, H.NP_AFTER[tag] // H.NB)
    _model_is_undisturbed(ck, e, P, n, (tag, kernel), first)
    e.close()
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# group E
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel,d', H.PROBLEMS)
def test_ensemble(kernel, d):
    from pybo_amd._lib import Engine
    P = H.problem(kernel, d)
    ck = Checks(('ensemble', kernel))
    n = H.ENS_N
    hyp = H.ENS_HYPERS
    # (the lead, whose option "prune" governs and whose workspace the ensemble uses, is a grown handle)
    members = [H.build('restride', P, hyp[0])[0], H.build('announced_unused', P, hyp[1], upto=n)[0], H.twin(P, n, hyp[2])]
    twins = [H.twin(P, n, h) for h in hyp]
    refs = [P.make_ref(P.X[:n], P.y[:n], h) for h in hyp]
    assert [m.N for m in members] == [n] * 3
    target = float(refs[0].mean_at_obs().max())
    for kind, param in H.ens_acqs(target):      # tests/test_gpu_ensemble_grid.py::test_ensemble_sweep_matches_oracle_members
        moments = kind == 'ucb'
        out = Engine.ensemble_sweep(members, kind, param, P.Zp, k=8, want_moments=moments)
        tw = Engine.ensemble_sweep(twins, kind, param, P.Zp, k=8, want_moments=moments)
        want, mu, s2 = H.ens_ref(refs, kind, param, P.Zp)
        tol = 1e-6 * np.abs(want) + 1e-9 * np.abs(want).max()
        ck.within('ensemble %s' % kind, out['acq'], want, tol)
        ck.within('ensemble %s against the twins' % kind, out['acq'], tw['acq'], tol)
        if moments:
            ck.within('ensemble mu', out['mu'], mu, 1e-6 * np.abs(mu) + 1e-9)
            ck.within('ensemble s2', out['s2'], s2, 1e-6 * np.abs(s2) + 1e-10)
        idx = gp_ref.topk_desc(out['acq'], 8)
        ck('ensemble %s top-k' % kind, np.array_equal(out['top_idx'], idx) and np.array_equal(out['top_val'], out['acq'][idx]))
        ck('ensemble %s winner' % kind, out['top_idx'][0] == int(np.argmax(want)) == tw['top_idx'][0])
    # the ensemble's selection-only sweep, pruned and plain, against the ranking of all its values
    full = Engine.ensemble_sweep(members, 'ei', target, P.Zsel, k=8)
    order = gp_ref.topk_desc(full['acq'], 8)
    for p in (1, 0):
        members[0].set_option('prune', p)
        r = Engine.ensemble_sweep(members, 'ei', target, P.Zsel, k=8, want_all=False)
        path = Engine.ensemble_prune_report(members, vectors=False)['path']
        print('ensemble selection-only prune %d: %s' % (p, path))
        ck('ensemble selection-only (prune %d)' % p, np.array_equal(r['top_idx'], order) and
           np.array_equal(r['top_val'], full['acq'][order]), (r['top_idx'], order))
        ck('ensemble selection-only (prune %d) path' % p, path in ('pruned', 'fell back') if p else path == 'plain', path)
    members[0].set_option('prune', -1)
    Z = P.Zp[:37]                               # ::test_ensemble_predict_equals_the_members_own_gradients
    got = Engine.ensemble_predict(members, Z)
    gtw = Engine.ensemble_predict(twins, Z)
    for i, (m, r) in enumerate(zip(members, refs)):
        own = m.predict(Z, grad=True)
        ck('ensemble_predict member %d == its own predict' % i, all(np.array_equal(got[j][i], own[j]) for j in range(4)))
        want = r.predict(Z, grad=True)
        for w, name in ((want, 'oracle'), ([g[i] for g in gtw], 'twin')):
            ck.within('ensemble_predict member %d mu (%s)' % (i, name), got[0][i], w[0], mu_tol(want[0], hyp[i][1]))
            ck.within('ensemble_predict member %d s2 (%s)' % (i, name), got[1][i], w[1], s2_tol(want[1], hyp[i][1]))
            if kernel != 'matern1':
                ck.within('ensemble_predict member %d dmu (%s)' % (i, name), got[2][i], w[2], 1e-8 + 1e-6 * np.abs(want[2]))
                ck.within('ensemble_predict member %d ds2 (%s)' % (i, name), got[3][i], w[3], 1e-8 + 1e-6 * np.abs(want[3]))
    for m in members + twins:
        m.close()
    ck.done()
