"""The quantity that guarantees a selection-only sweep (option "prune"), not only its outcome.

tests/test_gpu_prune.py shows the pruned top-k bit-equal to the plain one.  Here every one of the M candidates is held
against the invariants the proof rests on, read through gpx_prune_report (csrc/gpx_diag.h; option "prune_keep" keeps the
bound vector and the seed list as they were before the scatter):

  soundness   a candidate that was not evaluated has acq < tau strictly; ub >= acq wherever acq >= 1e-280, up to the
              rounding of the two acq_value calls (devmath_ref.acq_bound, per candidate); a NaN value has a NaN bound and
              a NaN bound survives or is a seed;
  truth       on 512 candidates (the 64 best, the 64 with the smallest ub - acq, the rest spread over the ranking), with
              the device's own T and a and the oracle's cross-covariances in long double (gp_ref.prune_truth):
              |mu_dev - mu_true| <= delta / 2, and ub >= EI(mu_true + delta / 2, sqrt(rho)) -- the proof gives
              |mu_est - mu_true| <= delta / 2, so the bound pass's EI(mu_est + delta, .) cannot lie below that -- hence also
              ub >= EI(mu_true, sqrt(rho)), within acq_bound;
  S, delta    S against the long-double S to (Np + 8) u relative: the products |U a| round once, a thread adds at most
              Np / 256 of them, the tree 8 levels, k_prune_delta the same again -- Np / 128 + 17 <= Np + 8 roundings for
              Np >= 128; delta == the fp64 expression of k_prune_delta (gp_ref.prune_delta) at the device's S;
  selection   recomputed in numpy: the seeds are G candidates in ascending index order, the first G in (24-bit key
              descending, index ascending) order; the bound vector after the scatter is the kept one with -inf at the seeds
              and at [0, done); tau is the k-th best value of the seeds; the survivors are flatnonzero(~(ub < tau (1 -
              1e-6))) in order; more survivors than cap <=> the sweep fell back and did all the work;
  outcome     values, indices, order array_equal to gp_ref.topk_desc(acq, k) and to prune = 0.

All assertions are exact inequalities or array_equal; the figures printed (-s) are the headroom table of DESIGN.md 2.1."""
import numpy as np
import pytest

import bench
import devmath_ref
from oracle import gp_ref
from helpers import synth_problem
from test_gpu_prune import _DevBuf, _dev

pytestmark = pytest.mark.gpu

TAU_MIN, SLACK = 1e-280, 1e-6


def _expected_sizes(N, k, M):
    """G, Gg, cap of api.hip sweep_core."""
    nP = (N + 127) // 128
    gen_tiles = max(1, 512 // ((nP + 1) // 2))
    G0 = 128 * min(32, gen_tiles)
    G = max(G0, (k + 127) // 128 * 128)
    return G, 128 * gen_tiles, max(G, M // 4)


def _engine(w, **opts):
    from pybo_amd._lib import Engine
    e = Engine(0)
    e.set_option('prune_keep', 1)
    for name, v in opts.items():
        e.set_option(name, v)
    e.fit(w['X'], w['y'], w['kernel'], w['ell'], w['rho'], w['sn2'], w['bias'])
    return e


def _ei_slack(mu, s2, p0, t):
    return devmath_ref.acq_bound('ei', mu, s2, p0, t)


def check_sweep(e, w, Z, k, prune=1, target=None, truth=True, label=''):
    """One pruned sweep of Z on the fitted engine e against every invariant of the module docstring; returns the
    report (with the figures of the headroom table added)."""
    X, rho, bias = w['X'], w['rho'], w['bias']
    N, M = e.N, len(Z)
    Np = (N + 127) // 128 * 128
    if target is None:
        target = e.mean_at_obs()[1]
    dZ = _dev(Z)
    buf = _DevBuf(3 * M)
    e.sweep_dev('ei', target, dZ.data_ptr(), M, 0, d_acq=buf.at(0), d_mu=buf.at(M), d_s2=buf.at(2 * M))
    e.sync()
    acq, mu, s2 = buf.numpy().reshape(3, M)
    assert e.prune_report()['path'] == 'plain'                     # a per-candidate call never prunes
    e.set_option('prune', 0)
    plain = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    e.set_option('prune', prune)
    e.timers(reset=True)
    got = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    flop = e.timers(reset=True)['sweep_trmm_flop']
    share = flop / (float(N) ** 2 * M)
    r = e.prune_report()
    r['share'] = share

    # ---- outcome --------------------------------------------------------------------------------------------------------
    want = gp_ref.topk_desc(acq, k)
    assert np.array_equal(got[1], want) and np.array_equal(got[0], acq[want], equal_nan=True), label
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[0], plain[0], equal_nan=True), label

    # ---- the decision ---------------------------------------------------------------------------------------------------
    G, Gg, cap = _expected_sizes(N, k, M)
    assert (r['M'], r['k'], r['G'], r['Gg'], r['cap']) == (M, k, G, Gg, cap), label
    legal = M >= 3 * G and 1e-100 <= rho < np.inf
    tried = legal and (prune == 1 or (M >= 32768 and Np >= 1024 and M >= Gg + 2 * G))
    if not tried:
        assert r['path'] == 'plain' and share == 1.0, label
        return r
    if prune < 0:
        gate = float(np.mean(s2[:Gg]))
        assert abs(r['gate_s2'] - gate) <= 1e-12 * rho, label
        if r['path'] == 'gate declined':
            assert r['gate_s2'] < rho / 64.0 and share == 1.0, label
            return r
        assert r['gate_s2'] >= rho / 64.0 and r['done'] == Gg, label
    else:
        assert r['done'] == 0 and np.isnan(r['gate_s2']), label
    assert r['path'] in ('pruned', 'fell back') and r['kept'] == 1, label
    done, tau, delta = r['done'], r['tau'], r['delta']
    ub, ubk, seeds, idx = r['ub'], r['ub_kept'], r['seed_idx'], r['idx']

    # ---- S and delta ----------------------------------------------------------------------------------------------------
    assert delta == gp_ref.prune_delta(r['S'], Np, rho, bias), label
    assert delta >= 0.0 and np.isfinite(delta), label

    # ---- selection ------------------------------------------------------------------------------------------------------
    assert np.all(np.isneginf(ubk[:done])), label
    assert len(seeds) == G and np.all(np.diff(seeds) > 0) and seeds[0] >= done and seeds[-1] < M, label
    keys = gp_ref.sel_key24(ubk)
    first = np.lexsort((np.arange(M), -keys))[:G]
    assert keys[first[-1]] == int(r['thr_key']), label
    assert np.array_equal(seeds, np.sort(first)), label
    expect = ubk.copy()
    expect[seeds] = -np.inf
    assert np.array_equal(ub, expect, equal_nan=True), label
    sv = acq[seeds]
    kth = sv[gp_ref.topk_desc(sv, k)[k - 1]]
    if np.isnan(kth):
        assert not (tau >= TAU_MIN), label                        # fewer than k seeds with a value: nothing is pruned
    else:
        assert tau == kth, label
    cut = tau * (1.0 - SLACK) if tau >= TAU_MIN else -np.inf
    surv = np.flatnonzero(~(ub < cut))
    assert r['nsurv'] == len(surv), label
    assert (r['path'] == 'fell back') == (len(surv) > cap), label
    if r['path'] == 'pruned':
        assert np.array_equal(idx, surv), label
        assert flop == float(N) ** 2 * (done + G + len(surv)), label
    else:
        assert share >= 1.0, label

    # ---- soundness, every candidate -------------------------------------------------------------------------------------
    skipped = np.ones(M, dtype=bool)
    skipped[:done] = False
    skipped[seeds] = False
    skipped[surv] = False
    if tau >= TAU_MIN:            # (also where the sweep fell back: the cut would have been sound had it been applied)
        assert np.all(acq[skipped] < tau), (label, int(np.sum(~(acq[skipped] < tau))))
    else:
        assert not skipped.any(), label
    live = np.arange(M) >= done
    nan_acq = np.isnan(acq)
    assert np.all(np.isnan(ubk[nan_acq & live])), label
    assert not np.any(np.isnan(ubk) & skipped), label
    need = live & (acq >= TAU_MIN)
    low = np.flatnonzero(need & ~(ubk >= acq))
    assert len(low) <= 4096, (label, len(low))                   # (each needs two 50-digit evaluations)
    # The second call's room belongs at (mu_est + delta, rho), and the report does not expose mu_est.  It is taken at
    # (mu_dev + delta, rho): the two means differ by at most delta (each lies within delta / 2 of mu_true), over which
    # acq_bound, smooth in z, changes by a relative O(delta / sqrt(rho)) -- nothing next to the bound itself.
    for n in low:
        t1 = devmath_ref.acq_truth('ei', mu[n], s2[n], target)
        t2 = devmath_ref.acq_truth('ei', mu[n] + delta, rho, target)
        room = _ei_slack(mu[n], s2[n], target, t1) + _ei_slack(mu[n] + delta, rho, target, t2)
        assert ubk[n] + room >= acq[n], (label, n, ubk[n], acq[n])
    fin = need & np.isfinite(ubk) & (acq > 0)
    r['min_ub_over_acq'] = float(np.min(ubk[fin] / acq[fin])) if fin.any() else np.nan

    # ---- the bound bounds the truth -------------------------------------------------------------------------------------
    r['mu_err_over_delta'] = np.nan
    if truth:                     # S alone is N^2 / 2 long-double products: checked at every N, padded block rows included
        T, a = e.get_matrix('T'), e.get_vectors()[0]
        S_ld = gp_ref.prune_S(T, a)
        assert abs(r['S'] - float(S_ld)) <= (Np + 8) * gp_ref.U53 * float(S_ld), (label, r['S'], float(S_ld))
    if truth and N <= 2049:
        ok = live & np.isfinite(acq) & np.isfinite(ubk)
        rank = gp_ref.topk_desc(np.where(ok, acq, -np.inf), int(ok.sum()))
        gap = np.where(ok, ubk - acq, np.inf)
        pick = np.unique(np.concatenate([rank[:64], np.argsort(gap, kind='stable')[:64],
                                         rank[np.linspace(0, len(rank) - 1, 512).astype(int)]]))
        pick = pick[ok[pick]]
        assert len(pick) >= min(128, int(ok.sum())), label
        Ks = gp_ref.kernel(gp_ref.KERNEL_IDS[w['kernel']], X, Z[pick], w['ell'], rho)
        mu_true = gp_ref.prune_truth(T, a, Ks, rho, bias)[0]
        err = np.abs(mu[pick].astype(np.longdouble) - mu_true).astype(float)
        r['mu_err_over_delta'] = float(err.max() / delta) if delta > 0 else np.inf
        assert np.all(err <= delta / 2), (label, r['mu_err_over_delta'])
        for j, n in enumerate(pick):
            for shift in (delta / 2, 0.0):
                t = devmath_ref.acq_truth('ei', float(mu_true[j]) + shift, rho, target)
                if t >= TAU_MIN:
                    assert ubk[n] + _ei_slack(float(mu_true[j]) + shift, rho, target, t) >= t, (label, n, shift)
    print('%-34s %-9s M %8d G %5d nsurv %8d share %.4f  S %.3e delta %.3e tau %.3e  max|mu-mu_true|/delta %.2e  '
          'min ub/acq %.9f' % (label, r['path'], M, G, r['nsurv'], share, r['S'], delta, tau, r['mu_err_over_delta'],
                               r['min_ub_over_acq']))
    return r


def _problem(N, d, M, kernel='se', seed=0, rho=1.3, bias=0.2, sn2_rel=1e-3):
    X, y, ell = synth_problem(N, d, seed=seed)
    if d > 8:
        ell = ell * np.sqrt(d / 4.0)                       # keep the data correlated in many dimensions
    rng = np.random.RandomState(seed + 100)
    return dict(X=X, y=bias + np.sqrt(rho) * y, ell=ell, rho=rho, sn2=sn2_rel * rho, bias=bias, kernel=kernel, N=N, d=d,
                Xc=rng.rand(M, d))


@pytest.mark.parametrize('kernel,d,N', [('se', 1, 128), ('matern5', 8, 129), ('matern3', 33, 1000), ('matern1', 64, 2049),
                                        ('se', 65, 300), ('matern5', 200, 300), ('matern1', 3, 1000), ('matern3', 2, 300)])
def test_bound_invariants_over_kernels_dimensions_and_sizes(kernel, d, N):
    M = 40961 if N * d <= 20000 else 20000
    w = _problem(N, d, M, kernel, seed=N + d)
    e = _engine(w)
    r = check_sweep(e, w, w['Xc'], 10, label='%s d=%d N=%d' % (kernel, d, N))
    assert r['path'] in ('pruned', 'fell back')
    if N >= 1000 and M >= 32768:
        check_sweep(e, w, w['Xc'], 64, prune=-1, label='%s d=%d N=%d auto' % (kernel, d, N))
    e.close()


@pytest.mark.parametrize('N,k,G', [(4100, 10, 3840), (8192, 10, 2048), (8192, 4096, 4096)])
def test_bound_invariants_where_the_generation_is_short_or_k_sets_the_seed_count(N, k, G):
    M = 3 * G + 1000
    w = _problem(N, 4, M, 'se', seed=N)
    assert _expected_sizes(N, k, M)[0] == G
    e = _engine(w)
    r = check_sweep(e, w, w['Xc'], k, label='N=%d k=%d' % (N, k))
    assert r['G'] == G and r['path'] in ('pruned', 'fell back')
    e.close()


@pytest.mark.parametrize('M', [3 * 4096 - 1, 3 * 4096, 3 * 4096 + 1, 40961, (1 << 20) + 4097, (1 << 21) + 1])
def test_bound_invariants_at_the_legality_edge_and_past_one_trip_of_the_scan(M):
    """N = 300 keeps these select-bound: G = 4096, so 3G - 1 must be plain; from 2^20 + 1 candidates on the scan of the
    per-block counts takes a second trip and its carry decides every offset of the later blocks."""
    w = _problem(300, 6, M, 'se', seed=11)
    e = _engine(w)
    k = 4096 if M > 1 << 20 else 10                     # (tau = the worst seed's value: survivors all over the index range)
    r = check_sweep(e, w, w['Xc'], k, label='M=%d' % M)
    if M == 3 * 4096 - 1:
        assert r['path'] == 'plain' and r['share'] == 1.0
    else:
        assert r['path'] in ('pruned', 'fell back')
        if M > 1 << 20:                                        # offsets behind the first 256 blocks come from the carry
            assert np.any(r['seed_idx'] >= 1 << 20) and (r['path'] == 'fell back' or np.any(r['idx'] >= 1 << 20))
    e.close()


@pytest.mark.parametrize('opts', [{}, {'refine_inverse': 1}, {'trtri_left': 1}], ids=['plain', 'refined', 'trtri_left'])
@pytest.mark.parametrize('noise', ['rel', 'lit'])
def test_bound_invariants_on_the_ill_conditioned_models(noise, opts):
    """Config B's inputs at sn2 = 1e-6 rho and at the literal 1e-6 (tests/test_gpu_illcond.py): a is huge, S with it, and
    the row-dot mean cancels."""
    M = 32768
    w = bench.make_workload('b', M)
    w['sn2'] = 1e-6 * w['rho'] if noise == 'rel' else 1e-6
    e = _engine(w, **opts)
    check_sweep(e, w, w['Xc'], 10, label='B %s %s' % (noise, sorted(opts)))
    check_sweep(e, w, w['Xc'], 64, prune=-1, label='B %s %s auto' % (noise, sorted(opts)))
    e.close()


@pytest.mark.parametrize('rho,bias_rel', [(1e-90, 1e6), (1e-6, -1e6), (1.0, 0.0), (1e8, 1e6), (1e8, -1e6), (1e-90, 0.0)])
def test_bound_invariants_over_scales_and_targets(rho, bias_rel):
    M = 30000
    bias = bias_rel * np.sqrt(rho)
    w = _problem(600, 3, M, 'se', seed=21, rho=rho, bias=bias)
    e = _engine(w)
    mu_obs, mx = e.mean_at_obs()
    for name, target in (('max', mx), ('below', float(mu_obs.min()) - 10.0 * np.sqrt(rho)), ('above', mx + 1e6 * np.sqrt(rho))):
        r = check_sweep(e, w, w['Xc'], 10, target=target, label='rho=%g bias=%g target %s' % (rho, bias, name))
        if name == 'above':
            assert not (r['tau'] >= TAU_MIN) and r['path'] == 'fell back'
    e.close()


def test_bound_invariants_after_appends_refits_and_on_interleaved_handles():
    M = 20000
    w = _problem(259, 3, M, 'matern5', seed=31)
    full = dict(w)
    w0 = dict(w, X=full['X'][:250], y=full['y'][:250])
    e = _engine(w0, sweep_cache=0)
    for n in range(250, 259):                                   # (256 -> 257 crosses a block: the append path grows it)
        assert e.append(full['X'][n], full['y'][n]), n
    assert e.N == 259
    appended = 9
    check_sweep(e, w, w['Xc'], 10, label='after %d appends' % appended)
    # the same handle refitted to a smaller, then a larger N and another d: the workspace is carved anew each time
    e2 = None
    for N, d, Mx in ((130, 2, 13000), (1500, 6, 45000), (259, 3, 20000)):
        wn = _problem(N, d, Mx, 'se', seed=N)
        e.fit(wn['X'], wn['y'], wn['kernel'], wn['ell'], wn['rho'], wn['sn2'], wn['bias'])
        check_sweep(e, wn, wn['Xc'], 64, label='refit N=%d d=%d' % (N, d))
        if e2 is None:
            w2 = _problem(700, 4, 30000, 'matern3', seed=77)
            e2 = _engine(w2)
        check_sweep(e2, w2, w2['Xc'], 10, label='second handle, after N=%d' % N)
    e.close()
    e2.close()


def test_bound_invariants_on_hard_candidate_sets():
    M, k = 30000, 10
    w = _problem(800, 3, M, 'se', seed=41)
    Z = w['Xc']
    # far from the data: ell = 1e-3 of the box, s2 == rho and ub ~ acq for every candidate (the tight regime)
    wf = dict(w, ell=np.full(3, 1e-3))
    e = _engine(wf)
    r = check_sweep(e, wf, Z, k, label='far from the data')
    # ... and a length scale at which the far candidates still see the data through a large a (s2 ~ rho, mu varies)
    wm = dict(w, ell=np.full(3, 0.02), sn2=1e-6 * w['rho'])
    e.fit(wm['X'], wm['y'], wm['kernel'], wm['ell'], wm['rho'], wm['sn2'], wm['bias'])
    check_sweep(e, wm, Z, k, label='short length scale')
    e.close()
    e = _engine(w)
    G = _expected_sizes(800, k, M)[0]
    # all candidates are copies of one point: every bound in one bin, the seeds are the first G by index
    r = check_sweep(e, w, np.repeat(Z[:1], M, axis=0), k, label='copies of one point')
    assert np.array_equal(r['seed_idx'], np.arange(G)) and r['path'] == 'fell back'
    # G + 1 rows with a NaN coordinate: every seed is NaN, tau is no number, the plain loop runs
    Zn = Z.copy()
    rows = np.random.RandomState(1).choice(M, G + 1, replace=False)
    Zn[rows, np.arange(G + 1) % 3] = np.nan
    r = check_sweep(e, w, Zn, k, label='G + 1 NaN rows')
    assert r['path'] == 'fell back' and not (r['tau'] >= TAU_MIN) and np.all(np.isnan(r['ub_kept'][r['seed_idx']]))
    # fewer NaN rows than seeds, and infinite coordinates (covariance 0: the prior at that candidate)
    Zi = Z.copy()
    Zi[rows[:50], 0] = np.nan
    Zi[rows[50:90], 1] = np.inf
    Zi[rows[90:130], 2] = -np.inf
    check_sweep(e, w, Zi, k, label='NaN and infinite coordinates')
    # bounds that differ only below the 12 mantissa bits of the key: a fine line through the best candidate; the
    # threshold bin holds far more than G candidates, and candidates of higher bins lie behind them in index order
    best = Z[int(e.sweep('ei', e.mean_at_obs()[1], Z, k=1, want_all=False)['top_idx'][0])]
    Zg = np.repeat(best[None, :], M, axis=0)
    Zg[:, 0] += np.linspace(-1e-5, 1e-5, M)
    Zg[M // 2:, 1] += np.linspace(0, 3e-3, M - M // 2)
    check_sweep(e, w, Zg, k, label='sub-key grid')
    check_sweep(e, w, Zg[::-1].copy(), 64, label='sub-key grid reversed')
    e.close()


@pytest.mark.parametrize('seed', range(48))
def test_seeded_random_campaign(seed):
    rng = np.random.RandomState(9000 + seed)
    kernel = ('se', 'matern5', 'matern3', 'matern1')[rng.randint(4)]
    N, d = int(rng.randint(130, 2501)), int(rng.randint(1, 41))
    M = int(rng.randint(12288, 70001))
    k = (1, 10, 64, 200, 4096)[rng.randint(5)]
    sn2_rel = 10.0 ** rng.uniform(-9, -1)
    w = _problem(N, d, M, kernel, seed=seed, sn2_rel=sn2_rel)
    e = _engine(w)
    _, mx = e.mean_at_obs()
    target = mx + (0.0, 0.0, -0.5, 0.3, 3.0)[rng.randint(5)] * np.sqrt(w['rho'])
    check_sweep(e, w, w['Xc'], k, prune=(1, 1, -1)[rng.randint(3)], target=target, truth=False,
                label='seed %d %s N=%d d=%d k=%d sn2=%.0e' % (seed, kernel, N, d, k, sn2_rel))
    e.close()
