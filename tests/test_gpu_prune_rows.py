"""The second bound of a selection-only sweep (option "prune_rows"): the variance bound
rho - q_R from the leading nR block rows of V = T K*, taken from a row-prefix launch of the sweep kernels.

What is held here, against a per-candidate call (acq, mu, s2 of every candidate) as in tests/test_gpu_prune_bound.py:

  bit-prefix  the prefix launch writes the full launch's bits: with nR = nP (N a multiple of 128) fmax(rho - q_R, 1e-100) is
              array_equal to the exact s2 of every first-level survivor; q_R is non-decreasing in nR and rho - q_R >= s2,
              exactly, for every nR -- on both default schedules (k_sweep_trmm_l from 32 block rows on, where the lower
              half's tiles walk k downwards, and k_sweep_trmm_w below), with nR on both sides of 2 mt < nP - 1;
  the bound   ub2 >= acq wherever acq >= 1e-280, up to the rounding of the two acq_value calls (devmath_ref.acq_bound);
              the second-level list is flatnonzero(~(ub2 < cut)) mapped through the first-level list;
  outcome     the top-k is array_equal to prune = 0 for k = 1, 10, 64; every survivor dropped at level two has acq < tau;
              sweep_trmm_flop == N^2 (done + G + nsurv2); with prune_rows = 0 the report and the flop are the single bound's;
  the rule    by size: nR = nP / 4 where M >= 32768, nP >= 32 and nsurv > Gg, and only there.

All assertions are exact inequalities or array_equal."""
import numpy as np
import pytest

import devmath_ref
from oracle import gp_ref
from test_gpu_prune import _DevBuf, _dev
from test_gpu_prune_bound import _engine, _expected_sizes, _problem, TAU_MIN, SLACK

pytestmark = pytest.mark.gpu


def _truth(e, Z, target):
    """acq, mu, s2 of every candidate from a call that asks for them (it never prunes)."""
    M = len(Z)
    dZ = _dev(Z)
    buf = _DevBuf(3 * M)
    e.sweep_dev('ei', target, dZ.data_ptr(), M, 0, d_acq=buf.at(0), d_mu=buf.at(M), d_s2=buf.at(2 * M))
    e.sync()
    acq, mu, s2 = buf.numpy().reshape(3, M)
    return dZ, acq, mu, s2


def _rows_expected(rows, N):
    nP = (N + 127) // 128
    return min(rows, nP, N // 128)


def check_rows(e, w, truth, target, k, rows, prune=1, expect_nR=None, label=''):
    """One pruned sweep with prune_rows = rows against the module docstring; returns the report."""
    dZ, acq, mu, s2 = truth
    rho, bias, N, M = w['rho'], w['bias'], e.N, len(acq)
    e.set_option('prune', 0)
    plain = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    e.set_option('prune', prune)
    e.set_option('prune_rows', rows)
    e.timers(reset=True)
    got = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    flop = e.timers(reset=True)['sweep_trmm_flop']
    r = e.prune_report()
    e.set_option('prune_rows', -1)

    want = gp_ref.topk_desc(acq, k)
    assert np.array_equal(got[1], want) and np.array_equal(got[0], acq[want], equal_nan=True), label
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[0], plain[0], equal_nan=True), label
    G = _expected_sizes(N, k, M)[0]
    if r['path'] == 'fell back':            # more first-level survivors than cap: the plain loop ran, no second level
        assert r['nsurv'] > r['cap'] and r['nR'] == 0 and r['nsurv2'] == 0 and flop >= float(N) ** 2 * M, label
        return r
    assert r['path'] == 'pruned' and r['kept'] == 1, (label, r['path'])
    done, tau, delta, idx = r['done'], r['tau'], r['delta'], r['idx']
    assert r['G'] == G and len(idx) == r['nsurv'], label
    if expect_nR is None:
        expect_nR = _rows_expected(rows, N) if r['nsurv'] > 0 else 0
    assert r['nR'] == expect_nR, (label, r['nR'], expect_nR)
    if r['nR'] == 0:
        # the single bound's path: report and count as before
        assert r['nsurv2'] == 0 and 'ub2' not in r, label
        assert flop == float(N) ** 2 * (done + G + r['nsurv']), label
        return r

    ub2, qR, idx2 = r['ub2'], r['qR'], r['idx2']
    assert len(ub2) == len(qR) == r['nsurv'] and len(idx2) == r['nsurv2'], label
    # ---- bit-prefix: q_R is a prefix of the exact chain's own sum ------------------------------------------------------------
    s2R = np.fmax(rho - qR, 1e-100)
    fin = ~np.isnan(mu[idx])                # (a NaN candidate: q is NaN and fmax returns the floor, on the device and here)
    assert np.all(qR[fin] >= 0.0), label
    assert np.all(s2R[fin] >= s2[idx][fin]), (label, int(np.sum(~(s2R[fin] >= s2[idx][fin]))))
    assert np.array_equal(np.isnan(qR), ~fin), label
    if r['nR'] * 128 == N:
        assert np.array_equal(s2R, s2[idx], equal_nan=True), label
    # ---- the bound -----------------------------------------------------------------------------------------------------------
    cut = tau * (1.0 - SLACK) if tau >= TAU_MIN else -np.inf
    keep = np.flatnonzero(~(ub2 < cut))
    assert np.array_equal(idx2, idx[keep]), label
    assert np.array_equal(np.isnan(ub2), ~fin), label
    need = acq[idx] >= TAU_MIN
    low = np.flatnonzero(need & ~(ub2 >= acq[idx]))
    assert len(low) <= 4096, (label, len(low))
    for j in low:                           # (the high-precision room of check_sweep, the second call at (mu + delta, s2R))
        n = idx[j]
        t1 = devmath_ref.acq_truth('ei', mu[n], s2[n], target)
        t2 = devmath_ref.acq_truth('ei', mu[n] + delta, s2R[j], target)
        room = devmath_ref.acq_bound('ei', mu[n], s2[n], target, t1) + devmath_ref.acq_bound('ei', mu[n] + delta, s2R[j], target, t2)
        assert ub2[j] + room >= acq[n], (label, n, ub2[j], acq[n])
    # ---- outcome and accounting ----------------------------------------------------------------------------------------------
    dropped = np.setdiff1d(idx, idx2)
    if tau >= TAU_MIN:
        assert np.all(acq[dropped] < tau), label
    else:
        assert len(dropped) == 0, label
    assert flop == float(N) ** 2 * (done + G + r['nsurv2']), label
    print('%-40s nR %2d nsurv %6d nsurv2 %6d  mean (rho - qR) / rho %.3f  low %d' %
          (label, r['nR'], r['nsurv'], r['nsurv2'], float(np.nanmean(rho - qR)) / rho if len(qR) else np.nan, len(low)))
    return r


# N, the rows asked for: nP = 32 and 33 on k_sweep_trmm_l (the down-rule is live: tiles with 2 mt < nP - 1), nR = 16 / 17 on
# both sides of it; nP = 11 on k_sweep_trmm_w; a request beyond N / 128 clamps (4100: 33 -> 32, 1300: 11 -> 10), and
# N = 1408 = 11 x 128 gives the w-kernel its nR = nP case.
# The third entry scales the length scales of the synthetic problem so that, by a CPU count of the first level beforehand, some
# 2000 candidates survive the prior-variance bound at k = 10 (cap = G: with denser data everything survives and the sweep falls
# back, with sparser data nothing does).
SHAPES = [(4096, (1, 2, 5, 16, 17, 32), 0.5), (4100, (1, 2, 5, 16, 17, 33), 0.5), (1300, (1, 3, 11), 0.85), (1408, (11,), 0.7)]
RULE_K = 10


def _scaled(N, M, scale, seed):
    w = _problem(N, 4, M, 'se', seed=seed)
    w['ell'] = w['ell'] * scale
    return w


@pytest.mark.parametrize('N,rows_list,scale', SHAPES, ids=['N%d' % s[0] for s in SHAPES])
def test_prefix_is_bit_exact_and_the_second_bound_is_sound(N, rows_list, scale):
    k = 10
    G = _expected_sizes(N, k, 1 << 20)[0]
    M = 3 * G + 1000
    w = _scaled(N, M, scale, N)
    e = _engine(w)
    target = e.mean_at_obs()[1]
    truth = _truth(e, w['Xc'], target)
    prev = None
    for rows in rows_list:
        r = check_rows(e, w, truth, target, k, rows, label='N=%d rows=%d' % (N, rows))
        assert r['path'] == 'pruned' and r['nsurv'] > 0
        if prev is not None:                # nR1 < nR2: the shorter prefix is no larger, element by element
            assert np.array_equal(prev['idx'], r['idx'])
            assert np.all(prev['qR'] <= r['qR'])
        prev = r
    for kk in (1, 64):
        check_rows(e, w, truth, target, kk, rows_list[1 if len(rows_list) > 1 else 0], label='N=%d k=%d' % (N, kk))
    # prune_rows = 0: exactly the single bound's report and count
    r0 = check_rows(e, w, truth, target, k, 0, label='N=%d rows=0' % N)
    assert r0['nR'] == 0 and np.array_equal(r0['idx'], prev['idx'])
    e.close()


def _rule_problem(N, M):
    return _scaled(N, M, 0.35, 4096)


def test_default_rule_fires_from_one_generation_of_survivors_on():
    """N = 4096, M = 65536, k = 10 (inputs counted on the CPU beforehand: some 7800 first-level survivors): more than Gg = 4096
    candidates survive the prior-variance bound, fewer than cap = 16384, so the rule takes nR = nP / 4 = 8 (the divisor the
    measurement on the headline workload chose: profiles/prune_rows_ab.md)."""
    N, M, k = 4096, 65536, RULE_K
    w = _rule_problem(N, M)
    e = _engine(w)
    target = e.mean_at_obs()[1]
    truth = _truth(e, w['Xc'], target)
    r = check_rows(e, w, truth, target, k, -1, expect_nR=8, label='rule N=4096 M=65536')
    assert r['nsurv'] > r['Gg'] == 4096 and r['nR'] == 32 // 4
    assert r['nsurv2'] <= r['nsurv']
    e.close()


# N, M, length-scale factor, k, more than Gg first-level survivors (CPU counts beforehand: 2714 of Gg = 4096; 5552 of 4096; 9718 of 8192):
# where more than a generation survives, M < 32768 or nP < 32 alone holds the rule back
SIBLINGS = [(4096, 20000, 0.35, 64, False), (4096, 32000, 0.35, 64, True), (2048, 65536, 0.5, 10, True)]


@pytest.mark.parametrize('N,M,scale,k,many', SIBLINGS, ids=['M20000', 'M32000', 'nP16'])
def test_default_rule_stays_out_below_its_sizes(N, M, scale, k, many):
    w = _scaled(N, M, scale, 4096)
    e = _engine(w)
    target = e.mean_at_obs()[1]
    truth = _truth(e, w['Xc'], target)
    r = check_rows(e, w, truth, target, k, -1, expect_nR=0, label='rule N=%d M=%d' % (N, M))
    assert r['path'] == 'pruned' and r['nR'] == 0
    assert (r['nsurv'] > r['Gg']) == many, (r['nsurv'], r['Gg'])
    e.close()


def test_adverse_inputs():
    N, k, rows = 4096, 10, 4
    G = _expected_sizes(N, k, 1 << 20)[0]
    M = 3 * G + 1000
    w = _scaled(N, M, 0.5, N)
    e = _engine(w)
    target = e.mean_at_obs()[1]
    Z = w['Xc']
    _, acq, _, _ = _truth(e, Z, target)
    best = gp_ref.topk_desc(acq, 3)
    # NaN coordinates (both signs of NaN, at the best candidate and elsewhere): a NaN bound is never cut, so whichever of them the
    # first level lists (the others are seeds: a NaN key sorts first) stay listed at the second; they rank last
    Zn = Z.copy()
    rng = np.random.RandomState(3)
    nan_rows = np.concatenate([best[:1], rng.choice(M, 40, replace=False)])
    Zn[nan_rows[::2], 1] = np.nan
    Zn[nan_rows[1::2], 2] = -np.nan
    truth = _truth(e, Zn, target)
    assert np.all(np.isnan(truth[1][nan_rows]))
    r = check_rows(e, w, truth, target, k, rows, label='NaN coordinates')
    listed = np.intersect1d(nan_rows, r['idx'])
    assert set(listed) <= set(r['idx2'])
    got = e.sweep_dev('ei', target, truth[0].data_ptr(), M, k)
    assert not set(nan_rows) & set(int(i) for i in got[1])
    # duplicated best candidates: ties resolved by index, as before
    Zd = Z.copy()
    Zd[[M - 5, 17, 9999]] = Z[best[0]]
    Zd[[123, M - 77]] = Z[best[1]]
    truth = _truth(e, Zd, target)
    check_rows(e, w, truth, target, k, rows, label='duplicates')
    got = e.sweep_dev('ei', target, truth[0].data_ptr(), M, k)
    assert set([17, 9999, M - 5, int(best[0])]) == set(int(i) for i in got[1][:4])
    e.close()
    # the leading rows far from every candidate: q_R is (next to) nothing, the second bound is the first and cuts nobody
    wf = dict(w, X=w['X'].copy())
    wf['X'][:rows * 128] += 40.0
    e = _engine(wf)
    target = e.mean_at_obs()[1]
    truth = _truth(e, Z, target)
    r = check_rows(e, wf, truth, target, k, rows, label='far leading rows')
    assert r['nsurv2'] == r['nsurv'] > 0 and np.all(r['qR'] <= 1e-200 * wf['rho'])
    e.close()


# nR, length-scale factor, k: a CPU count beforehand gives 1304 and 510 first-level survivors (cap 4096)
WITNESS = [(2, 0.8, 64), (17, 0.5, 10)]


@pytest.mark.parametrize('nR,scale,k', WITNESS, ids=['nR2', 'nR17'])
def test_prefix_bits_equal_the_full_launch_below_nP(nR, scale, k):
    """A witness of the bits at nR < nP: observations [nR 128, N) lie so far from the leading ones and from every candidate that
    those covariances are exactly 0.  The Gram matrix is block diagonal, so are its factor and T, the block rows rb >= nR of V are
    exactly 0 and the full launch's q is its own sum over rb < nR: fmax(rho - q_R, 1e-100) of the row-prefix launch must be
    array_equal to the exact s2 -- which it is only if the prefix launch writes the full launch's bits into Qp[rb < nR] (nR = 2:
    tiles that walk k downwards under the rule of nP = 32; nR = 17: one that does not among them)."""
    N = 4096
    M = 3 * _expected_sizes(N, k, 1 << 20)[0] + 1000
    w = _scaled(N, M, scale, N)
    w['X'] = w['X'].copy()
    w['X'][nR * 128:] += 40.0
    e = _engine(w)
    target = e.mean_at_obs()[1]
    truth = _truth(e, w['Xc'], target)
    r = check_rows(e, w, truth, target, k, nR, label='witness nR=%d' % nR)
    assert r['path'] == 'pruned' and r['nR'] == nR < 32 and r['nsurv'] > 0
    s2 = truth[3][r['idx']]
    assert np.array_equal(np.fmax(w['rho'] - r['qR'], 1e-100), s2)
    assert np.any(s2 < w['rho'])                       # (the leading rows do explain variance: the equality is about real sums)
    e.close()
