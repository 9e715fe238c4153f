"""Power conditions of tests/test_gpu_handle_history.py, from the oracle alone: what a handle's history adds to the model must be
far larger than the tolerances the device is compared at, so that a dropped row, a stale row, a wrong stride after the rotation or
a padded row counted as data cannot hide inside one.  These are conditions on the INPUTS (tests/history_ref.py): if a shape
changes, choose inputs that meet them again."""
import numpy as np
import pytest

import batch_ref
import history_ref as H
from history_ref import RHO
from oracle import gp_ref
from helpers import s2_tol, mu_tol

FACTOR, OF = 100.0, H.N_CAND
APPENDED = [c for c in H.cells() if H.HISTORIES[c[0]][1] > H.HISTORIES[c[0]][0]]
EMPTY = [c for c in H.cells() if c[0] in H.TRAILING_EMPTY]


def _moved_s2(P, n_from, n_to):
    before, after = P.ref(n_from)[2], P.ref(n_to)[2]
    return int(np.sum(np.abs(after - before) > FACTOR * s2_tol(after, RHO)))


@pytest.mark.parametrize('tag,kernel,d', APPENDED)
def test_the_appended_observations_move_the_posterior_far_beyond_the_tolerances(tag, kernel, d):
    P = H.problem_of(tag, kernel, d)
    n0, n = H.HISTORIES[tag]
    whole, last = _moved_s2(P, n0, n), _moved_s2(P, n - 1, n)
    l0, l1 = P.ref(n0)[0].loglikelihood(), P.ref(n)[0].loglikelihood()
    print('%s %s: whole block moves %d, last point %d of %d candidates; loglik %.6g -> %.6g' % (tag, kernel, whole, last, OF, l0, l1))
    # the whole appended block -- where it IS a block: 'announced_then_other' appends one point, whose condition is the next line's
    # (no single observation of the Matern-1/2 problem moves more than 58 candidates)
    assert whole >= 100 or n == n0 + 1
    assert last >= 10                           # the last appended point alone
    assert abs(l1 - l0) > 1e-3 * abs(l1)


@pytest.mark.parametrize('tag,kernel,d', EMPTY)
def test_a_padded_row_read_as_data_moves_the_posterior_far_beyond_the_tolerances(tag, kernel, d):
    P = H.problem_of(tag, kernel, d)
    n = H.HISTORIES[tag][1]
    r, mu, _ = P.ref(n)
    ph = P.phantom(n)
    moved = int(np.sum(np.abs(ph.predict(P.Zp)[0] - mu) > FACTOR * mu_tol(mu, RHO)))
    l0, l1 = r.loglikelihood(), ph.loglikelihood()
    print('%s %s: a phantom (0, 0) moves mu at %d of %d candidates; loglik %.6g -> %.6g' % (tag, kernel, moved, OF, l0, l1))
    assert moved >= 100
    assert abs(l1 - l0) > 1e-3 * abs(l0)
    # the same for the raw readers: every one of the nine log-likelihoods and the feature Gram see the phantom
    raw = P.raw_ref(n)
    args = P.raw_args()
    for th, want in zip(args['thetas'], raw['loglik_batch']):
        ph.set_hyper_vector(th)
        assert abs(ph.loglikelihood() - want) > 1e3 * 1e-9 * abs(want)
    W, b, _ = args['draws'][30]
    c = np.cos(b[0])                            # the phantom's feature row: cos(0 . w + b)
    assert np.abs(np.outer(c, c)).max() > 1e3 * (1e-11 * np.abs(raw['rff_gram_A_30']).max() + 1e-10)


@pytest.mark.parametrize('tag,kernel,d', H.cells())
def test_selections_are_decided_by_more_than_the_tolerances(tag, kernel, d):
    """Admission of the comparisons of ORDER: the oracle's best candidate under each acquisition leads the second by more than 1e-5
    relative (ten times the 1e-6 the values are compared at), and so does every round of the greedy batch (batch_ref.MIN_MARGIN)."""
    P = H.problem_of(tag, kernel, d)
    n = H.HISTORIES[tag][1]
    r, mu, s2 = P.ref(n)
    target = float(r.mean_at_obs().max())
    for kind, param in H.acqs(target):
        v = batch_ref.acq_from_moments(kind, param, mu, s2) if kind != 'mean' else mu
        o = gp_ref.topk_desc(v, 2)
        assert v[o[0]] - v[o[1]] > 1e-5 * abs(v[o[0]]), (kind, v[o])
    sk = P.survivor_k(n)
    print(tag, kernel, 'selection-only sweep with survivors: (k, predicted survivors) =', sk)
    assert sk is not None                       # a k at which the pruned sweep has survivors to evaluate (Problem.survivor_k)
    g = P.greedy(n)[1]
    print(tag, kernel, 'greedy margins', g['margin'])
    assert g['margin'].min() >= batch_ref.MIN_MARGIN


@pytest.mark.parametrize('kernel,d', H.PROBLEMS)
def test_the_ensembles_selection_is_decided_too(kernel, d):
    P = H.problem(kernel, d)
    refs = [P.make_ref(P.X[:H.ENS_N], P.y[:H.ENS_N], hyp) for hyp in H.ENS_HYPERS]
    target = float(refs[0].mean_at_obs().max())
    for kind, param in H.ens_acqs(target):
        v = H.ens_ref(refs, kind, param, P.Zp)[0]
        o = gp_ref.topk_desc(v, 2)
        assert v[o[0]] - v[o[1]] > 1e-5 * abs(v[o[0]]), (kind, v[o])
