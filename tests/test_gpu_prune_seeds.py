"""Seeds sized to the chip (pybo_amd/csrc/api.hip: prune_geom, PRUNE_SEEDS_MIN_NP): where the seeds'
exact launch can run on narrow tiles -- M >= 32768 candidates over at least 48 block rows on the default schedule, option sweep_cols
not 128 -- a selection-only sweep takes G = max(32 max(1, 256 // pairs), ceil128(k)) seeds, pairs = (nP + 1) // 2, instead of a wide
generation.  Gg, the form of cap and of the conditions on M, the gate, the hint rule and the flow do not change.

What is held here, against a per-candidate call on the same engine (acq, mu, s2 of every candidate), as tests/test_gpu_prune_bound.py
and tests/test_gpu_prune_rows.py hold the old sizes:

  inside the rule   top-k array_equal to prune = 0 and to the per-candidate call; G, Gg, cap by the formula written HERE; the seeds are
                    the first G in (24-bit key descending, index ascending) order; tau is the k-th best exact seed value; the first-
                    and second-level lists are the flatnonzero sets; every skipped candidate has acq < tau;
                    sweep_trmm_flop == N^2 (done + G + nsurv2);
  just outside      N = 6016 (47 block rows), M = 32767, sweep_cols = 128: check_rows of test_gpu_prune_rows.py, i.e. the old sizes and
                    the old accounting, unchanged;
  the hint          a carried gate decision still skips the gate of the next sweep inside the rule and is dropped by
                    gpx_set_option("sweep_cols", ...);
  the ensemble      three members, top-k alone through gpx_ensemble_sweep_dev: array_equal to prune = 0 (the ensemble keeps the old G).

All assertions are exact inequalities or array_equal."""
import numpy as np
import pytest

from oracle import gp_ref
from test_gpu_prune import _dev
from test_gpu_prune_bound import _engine, _expected_sizes, TAU_MIN, SLACK
from test_gpu_prune_rows import _scaled, _truth, check_rows

pytestmark = pytest.mark.gpu

N_IN, M_IN = 6144, 32768


def _seed_sizes(N, k, M, narrow=True):
    """G, Gg, cap of api.hip prune_geom under the rule of this file."""
    nP = (N + 127) // 128
    G, Gg, cap = _expected_sizes(N, k, M)
    if narrow and M >= 32768 and nP >= 48:
        G = max(32 * max(1, 256 // ((nP + 1) // 2)), (k + 127) // 128 * 128)
        cap = max(G, M // 4)
    return G, Gg, cap


def test_the_formula_at_the_sizes_of_this_file():
    assert _seed_sizes(N_IN, 10, M_IN) == (320, 2688, 8192) and _seed_sizes(N_IN, 300, M_IN)[0] == 384
    assert _seed_sizes(8192, 10, 1 << 20) == (256, 2048, 1 << 18)
    assert _seed_sizes(6016, 10, M_IN) == _expected_sizes(6016, 10, M_IN) == (2688, 2688, 8192)
    assert _seed_sizes(N_IN, 10, M_IN - 1) == _expected_sizes(N_IN, 10, M_IN - 1)


# k -> (length-scale factor of the synthetic problem, prune_rows).  A CPU count beforehand (float64 numpy, ub = EI(mu, sqrt(rho)) without
# the device's margins, so the device's lists are a little longer) at N = 6144, M = 32768, seed 6144, with 320 seeds:
#   k = 10, factor 0.35: tau 1.416e-01, 3632 first-level survivors (more than Gg = 2688: the second bound runs by its own rule with
#                        nR = 12), 420 of them at the second level -- the final exact launch has 420 columns: narrow;
#   k = 64: the k best sit deeper in the ranking by ub, so the lists are longer at every factor; wherever more than Gg survive the first
#                        level, more than 1024 survive the second (0.26: 2929 and 1047; 0.30: 4973 and 1283) and the final launch is
#                        wide.  So this case asks for the rule's nR = nP / 4 = 12 rows itself (prune_rows = 12: the same flow wherever
#                        the first level pruned) at factor 0.24: tau 1.748e-01, 1787 first-level survivors, 682 at the second level.
CASES = {10: (0.35, -1), 64: (0.24, 12)}

_FITTED = {}


def _fitted(scale):
    if scale not in _FITTED:
        w = _scaled(N_IN, M_IN, scale, N_IN)
        e = _engine(w)
        target = e.mean_at_obs()[1]
        _FITTED[scale] = (w, e, target, _truth(e, w['Xc'], target))
    w, e, target, truth = _FITTED[scale]
    for name, v in (('prune', -1), ('prune_rows', -1), ('sweep_cols', -1)):
        e.set_option(name, v)
    return w, e, target, truth


def check_seeds(e, truth, target, k, prune, rows, label):
    """One pruned sweep inside the rule against the module docstring; returns the report."""
    dZ, acq, mu, s2 = truth
    N, M = e.N, len(acq)
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
    assert np.array_equal(got[1], want) and np.array_equal(got[0], acq[want]), label
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[0], plain[0]), label
    G, Gg, cap = _seed_sizes(N, k, M)
    assert (r['M'], r['k'], r['G'], r['Gg'], r['cap']) == (M, k, G, Gg, cap), (label, r['G'], r['Gg'], r['cap'])
    assert r['path'] == 'pruned' and r['kept'] == 1, (label, r['path'], r['nsurv'])
    done, tau = r['done'], r['tau']
    assert done == (Gg if prune < 0 and not r['gate_hint'] else 0), (label, done)
    ub, ubk, seeds, idx = r['ub'], r['ub_kept'], r['seed_idx'], r['idx']
    # the seeds: the first G by key
    assert np.all(np.isneginf(ubk[:done])), label
    assert len(seeds) == G and np.all(np.diff(seeds) > 0) and seeds[0] >= done and seeds[-1] < M, label
    keys = gp_ref.sel_key24(ubk)
    first = np.lexsort((np.arange(M), -keys))[:G]
    assert np.array_equal(seeds, np.sort(first)), label
    # tau: the k-th best exact seed value
    sv = acq[seeds]
    assert tau == sv[gp_ref.topk_desc(sv, k)[k - 1]] and tau >= TAU_MIN, label
    # the first-level list
    cut = tau * (1.0 - SLACK)
    expect = ubk.copy()
    expect[seeds] = -np.inf
    assert np.array_equal(ub, expect), label
    surv = np.flatnonzero(~(ub < cut))
    assert np.array_equal(idx, surv) and r['nsurv'] == len(surv), label
    assert G < r['nsurv'] <= cap, (label, r['nsurv'])
    # the second-level list
    nP = (N + 127) // 128
    assert r['nR'] == nP // 4 and (rows > 0 or r['nsurv'] > Gg), (label, r['nR'], r['nsurv'])
    ub2, idx2 = r['ub2'], r['idx2']
    assert np.array_equal(idx2, idx[np.flatnonzero(~(ub2 < cut))]) and r['nsurv2'] == len(idx2), label
    assert 0 < r['nsurv2'] <= 1024, (label, r['nsurv2'])              # the final exact launch runs and is narrow
    # soundness and accounting
    skipped = np.ones(M, dtype=bool)
    skipped[:done] = False
    skipped[seeds] = False
    skipped[idx2] = False
    assert np.all(acq[skipped] < tau), (label, int(np.sum(~(acq[skipped] < tau))))
    assert flop == float(N) ** 2 * (done + G + r['nsurv2']), (label, flop / float(N) ** 2)
    print('%-28s G %4d done %5d tau %.3e nsurv %6d nR %2d nsurv2 %5d gate_s2 %.3e' %
          (label, G, done, tau, r['nsurv'], r['nR'], r['nsurv2'], r['gate_s2']))
    return r


@pytest.mark.parametrize('prune', [1, -1], ids=['forced', 'by_rule'])
@pytest.mark.parametrize('k', sorted(CASES))
def test_inside_the_rule(k, prune):
    scale, rows = CASES[k]
    w, e, target, truth = _fitted(scale)
    check_seeds(e, truth, target, k, prune, rows, 'k=%d prune=%d' % (k, prune))


def test_a_carried_hint_skips_the_gate_and_an_option_call_drops_it():
    k = 10
    w, e, target, truth = _fitted(CASES[k][0])
    check_seeds(e, truth, target, k, -1, -1, 'hint: checked sweep')       # (its option calls drop whatever is carried, before and after)
    dZ, M = truth[0], len(truth[1])
    e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    r1 = e.prune_report()
    assert not r1['gate_hint'] and r1['done'] == r1['Gg'] and r1['path'] == 'pruned' and r1['nsurv'] <= r1['cap'] // 2
    got2 = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    r2 = e.prune_report()
    assert r2['gate_hint'] and r2['done'] == 0 and r2['path'] == 'pruned' and r2['G'] == r1['G'] == 320
    want = gp_ref.topk_desc(truth[1], k)
    assert np.array_equal(got2[1], want) and np.array_equal(got2[0], truth[1][want])
    e.set_option('sweep_cols', -1)
    got3 = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    r3 = e.prune_report()
    assert not r3['gate_hint'] and r3['done'] == r3['Gg'] and r3['path'] == 'pruned'
    assert np.array_equal(got3[1], want) and np.array_equal(got3[0], got2[0])


OUTSIDE = [(6016, M_IN, -1), (N_IN, M_IN - 1, -1), (N_IN, M_IN, 128)]


@pytest.mark.parametrize('N,M,cols', OUTSIDE, ids=['nP47', 'M32767', 'sweep_cols128'])
def test_just_outside_the_rule_the_sizes_and_the_accounting_are_the_old_ones(N, M, cols):
    k = 10
    if N == N_IN:
        w, e, target, truth = _fitted(CASES[k][0])
        if M < M_IN:
            truth = _truth(e, w['Xc'][:M], target)
    else:
        w = _scaled(N, M, CASES[k][0], N_IN)
        e = _engine(w)
        target = e.mean_at_obs()[1]
        truth = _truth(e, w['Xc'], target)
    e.set_option('sweep_cols', cols)
    assert _seed_sizes(N, k, M, narrow=cols != 128) == _expected_sizes(N, k, M)
    # check_rows holds G == _expected_sizes(...)[0], the lists and the flop; the second bound's own rule (untouched) says whether nR > 0
    e.set_option('prune', 1)
    e.sweep_dev('ei', target, truth[0].data_ptr(), M, k)
    nsurv, nP = e.prune_report(vectors=False)['nsurv'], (N + 127) // 128
    expect_nR = nP // 4 if M >= 32768 and nsurv > _expected_sizes(N, k, M)[1] else 0
    r = check_rows(e, w, truth, target, k, -1, expect_nR=expect_nR, label='outside N=%d M=%d sweep_cols=%d' % (N, M, cols))
    assert r['nsurv'] == nsurv
    assert r['path'] == 'pruned' and r['G'] == _expected_sizes(N, k, M)[0] == 2688
    e.set_option('sweep_cols', -1)
    if N != N_IN:
        e.close()


def test_three_member_ensemble_top_k_alone():
    from pybo_amd._lib import Engine
    from test_gpu_ens_prune import _dev_cand
    k = 10
    scale = CASES[k][0]
    w, e0, target, truth = _fitted(scale)
    others = [_engine(dict(w, ell=w['ell'] * f, rho=w['rho'] * g)) for f, g in ((0.9, 1.2), (1.1, 0.9))]
    engines = [e0] + others
    Z = _dev_cand(w['Xc'])
    out = {}
    for prune in (0, 1):
        e0.set_option('prune', prune)
        for e in engines:
            e.timers(reset=True)
        r = Engine.ensemble_sweep(engines, 'ei', target, Z, k=k, want_all=False)
        work = sum(e.timers(reset=True)['sweep_trmm_flop'] for e in engines) / (3 * float(N_IN) ** 2 * M_IN)
        out[prune] = (r['top_val'], r['top_idx'], work, Engine.ensemble_prune_report(engines))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    rep = out[1][3]
    # (the ensemble keeps the wide generation of seeds: api.hip, ensemble_core; its members' short launches are narrow all the same)
    assert rep['path'] == 'pruned' and rep['G'] == _expected_sizes(N_IN, k, M_IN)[0] == 2688, (rep['path'], rep['G'])
    assert out[0][2] == 1.0 and out[1][2] == (rep['G'] + rep['nsurv']) / float(M_IN) < 0.5, (out[0][2], out[1][2])
    for e in others:
        e.close()


def teardown_module(module):
    for w, e, target, truth in _FITTED.values():
        e.close()
    _FITTED.clear()
