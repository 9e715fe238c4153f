"""Selection-only ENSEMBLE sweeps: an EI ensemble sweep that returns only its top-k evaluates the
members exactly only where the mean of their bounds can reach the k-th best value.  The pruned path must return BIT FOR
BIT what the loop over every candidate returns, must really leave the work out, and its bound must hold on every
candidate.  Every comparison of results is array_equal; the shapes are those of ens_prune_cases.py (the oracle's survivor
counts for them: test_ens_prune_cpu.py)."""
import numpy as np
import pytest

from oracle import gp_ref
import ens_prune_cases as cases
from test_gpu_prune import _dev

pytestmark = pytest.mark.gpu

_ENS = {}


def _ensemble(name):
    """The case's fitted member engines (once per session) and its problem."""
    if name not in _ENS:
        from pybo_amd._lib import Engine
        p = cases.problem(name)
        N = p['N']
        engines = []
        for sn2, rho, ell, bias in p['hypers']:
            e = Engine(0)
            e.fit(p['X'][:N], p['y'][:N], p['kernel'], ell, rho, sn2, bias)
            for j in range(N, N + p['app']):
                assert e.append(p['X'][j], float(p['y'][j]))
            engines.append(e)
        _ENS[name] = (p, engines)
    p, engines = _ENS[name]
    for e in engines:
        e.set_option('prune', -1)
        e.set_option('sweep_cache', -1)
    return p, engines


def _dev_cand(Z):
    """Host candidates copied to the device, in the shape Engine.ensemble_sweep takes for its device form."""
    from pybo_amd._lib import DeviceGrid

    class Cand(DeviceGrid):
        def __init__(self, Z):
            self._g = None
            self._buf = _dev(Z)
            self.shape = Z.shape
            self.ptr = self._buf.data_ptr()

        def close(self):
            pass
    return Cand(Z)


def _work(p, engines, m):
    """(the members' algorithmic sweep flop since the last call) / (n N^2 M)"""
    N = float(p['N'] + p['app'])
    return sum(e.timers(reset=True)['sweep_trmm_flop'] for e in engines) / (len(engines) * N * N * m)


def _sweep(p, engines, Z, k, prune, acq='ei', param=None, dev=True):
    from pybo_amd._lib import Engine
    engines[0].set_option('prune', prune)
    _work(p, engines, 1)
    r = Engine.ensemble_sweep(engines, acq, p['target'] if param is None else param, _dev_cand(Z) if dev else Z, k=k, want_all=False)
    return r['top_val'], r['top_idx'], _work(p, engines, len(Z)), Engine.ensemble_prune_report(engines)


def _all_values(p, engines, Z, acq='ei', param=None):
    from pybo_amd._lib import Engine
    r = Engine.ensemble_sweep(engines, acq, p['target'] if param is None else param, Z, k=0, want_all=True)
    assert Engine.ensemble_prune_report(engines)['path'] == 'plain'        # a per-candidate call never prunes
    return r['acq']


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


def _topk_of(vals, k):
    idx = gp_ref.topk_desc(vals, k)
    return vals[idx], idx


_VALUES = {}


def _values(name):
    if name not in _VALUES:
        p, engines = _ensemble(name)
        _VALUES[name] = _all_values(p, engines, p['Z'])
    return _VALUES[name]


@pytest.mark.parametrize('k', cases.KS)
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_pruned_and_plain_paths_agree_and_the_work_goes_away(name, k):
    """prune = 0 against prune = 1 on the lead, device form and host form, against the top-k of the want_all values; the
    report says `pruned` and the members' sweep flop fall below n N^2 M (exactly n N^2 M with prune = 0)."""
    vals = _values(name)
    p, engines = _ensemble(name)
    want = _topk_of(vals, k)
    for dev in (True, False):
        plain = _sweep(p, engines, p['Z'], k, 0, dev=dev)
        pruned = _sweep(p, engines, p['Z'], k, 1, dev=dev)
        assert _same(plain, pruned) and _same(pruned, want), (name, k, dev)
        print('%s k=%d %s: share %.4f against %.4f, survivors %d, tau %.4g' %
              (name, k, 'dev' if dev else 'host', pruned[2], plain[2], pruned[3]['nsurv'], pruned[3]['tau']))
        assert plain[3]['path'] == 'plain' and plain[2] == 1.0
        assert pruned[3]['path'] == 'pruned' and pruned[2] < 1.0
        assert pruned[3]['G'] == cases.G and pruned[3]['cap'] == cases.cap_of(len(vals)) and pruned[3]['nsurv'] <= pruned[3]['cap']
        # the share is the seeds' and the survivors', nothing else
        assert pruned[2] == pytest.approx((cases.G + pruned[3]['nsurv']) / float(len(vals)), rel=1e-12)


def _check_bound(rep, vals):
    """The report's bound vector against every candidate's exact value."""
    ub, tau = rep['ub'], rep['tau']
    cut = tau * (1.0 - 1e-6) if tau >= 1e-280 else -np.inf
    surv = np.flatnonzero(~(ub < cut))
    if rep['path'] == 'pruned':
        assert np.array_equal(rep['idx'], surv)             # the survivor list, recomputed from ub and tau
    else:
        assert len(surv) == rep['nsurv'] > rep['cap']
    seen = np.isneginf(ub)                                   # evaluated as gate or seed
    assert seen[:rep['done']].all() and seen.sum() == rep['done'] + rep['G']
    left_out = ~seen
    left_out[surv] = False
    assert np.all(vals[left_out] < tau)                      # not evaluated => it cannot be among the k best
    fin = np.isfinite(ub)
    assert np.all(ub[fin] >= vals[fin])
    assert not np.isnan(vals[fin | np.isposinf(ub)]).any()   # a NaN value has a NaN bound (or was evaluated: NaN keys seed first)
    assert np.isnan(vals[np.isnan(ub)]).all()
    return surv


@pytest.mark.parametrize('name,k', [(n, 10) for n in sorted(cases.CASES)] + [('m5_n3_d5', 200)])
def test_the_ensemble_bound_holds_on_every_candidate(name, k):
    vals = _values(name)
    p, engines = _ensemble(name)
    got = _sweep(p, engines, p['Z'], k, 1)
    rep = got[3]
    assert rep['path'] == 'pruned' and rep['done'] == 0 and np.isnan(rep['gate'])
    surv = _check_bound(rep, vals)
    if (name, k) == ('m5_n3_d5', 200):
        assert len(surv) > 0                                 # (the case that exercises the survivors' gather and scatter)
    # tau is the k-th best of the seeds' exact values
    seeds = np.flatnonzero(np.isneginf(rep['ub']))
    assert rep['tau'] == np.sort(vals[seeds])[::-1][k - 1]
    # one delta per member: the very delta_m = 8 (Np + 16) 2^-53 (rho_m S_m + |bias_m|) of that member's own selection-only sweep
    assert rep['delta'].shape == (p['n'],) and np.all(rep['delta'] > 0)
    dZ = _dev(p['Z'])
    for e, dm in zip(engines, rep['delta']):
        e.set_option('prune', 1)
        e.sweep_dev('ei', p['target'], dZ.data_ptr(), len(vals), k)
        own = e.prune_report(vectors=False)
        assert own['path'] in ('pruned', 'fell back') and own['delta'] == dm


def test_edge_inputs():
    from pybo_amd._lib import Engine
    name, k = 'se_n3', 10
    vals = _values(name)
    p, engines = _ensemble(name)
    Z = p['Z']

    def both(Zc, acq='ei', param=None, kk=k):
        v = _all_values(p, engines, Zc, acq, param)
        res = [_sweep(p, engines, Zc, kk, pr, acq, param) for pr in (0, 1)]
        assert _same(res[0], res[1])
        clean = np.where(np.isnan(v), -np.inf, v)
        assert np.array_equal(res[1][1], gp_ref.topk_desc(clean, kk))
        return v, res[1]

    best = gp_ref.topk_desc(vals, 3)
    # a NaN coordinate: ranks last, everything else as before; the bound still holds on every candidate
    Zn = Z.copy()
    Zn[best[0], 1] = np.nan
    Zn[9000, 0] = np.nan
    v, res = both(Zn)
    assert np.isnan(v[best[0]]) and np.isnan(v[9000]) and int(best[0]) not in res[1]
    assert res[3]['path'] == 'pruned'
    _check_bound(res[3], v)
    # duplicates of one candidate at the top: ties resolved by index
    Zd = Z.copy()
    Zd[[12000, 17, 6999]] = Z[best[0]]
    Zd[[123, 11000]] = Z[best[1]]
    v, res = both(Zd)
    assert res[3]['path'] == 'pruned'
    assert sorted([17, 6999, 12000, int(best[0])]) == [int(i) for i in res[1][:4]]
    # a target far above every mean: every EI underflows to 0, tau = 0 prunes nothing and the plain loop runs after the seeds
    v, res = both(Z, param=p['target'] + 1e6)
    assert np.all(v == 0.0) and np.array_equal(res[1], np.arange(k))
    assert res[3]['path'] == 'fell back' and res[3]['tau'] == 0.0 and res[3]['nsurv'] > res[3]['cap']
    assert res[2] == pytest.approx(1.0 + cases.G / float(len(Z)), rel=1e-12)
    # M = 3 G is legal, 3 G - 1 is not
    for m, legal in ((3 * cases.G, True), (3 * cases.G - 1, False)):
        v, res = both(Z[:m])
        assert (res[3]['path'] == 'pruned') == legal and (res[3]['path'] == 'plain') == (not legal), (m, res[3]['path'])
        assert (res[2] < 1.0) == legal
    # a member with its sweep cache on: the plain loop, which fills that cache as ever
    engines[1].set_option('sweep_cache', 1)
    v, res = both(Z)
    assert res[3]['path'] == 'plain' and res[2] == 1.0 and engines[1].sweep_cache_size() == len(Z)
    engines[1].set_option('sweep_cache', -1)
    # PI, UCB and the mean: the plain loop
    for acq, param in (('pi', p['target']), ('ucb', 2.0), ('mean', None)):
        v, res = both(Z, acq, param)
        assert res[3]['path'] == 'plain' and res[2] == 1.0, acq
    # a refused call clears the record
    with pytest.raises(Exception):
        Engine.ensemble_sweep(engines, 'ei', p['target'], Z, k=4097, want_all=False)
    with pytest.raises(Exception):
        Engine.ensemble_prune_report(engines)


def test_an_ensemble_of_one_equals_the_member_s_own_sweep():
    name = 'se_n1'
    p, engines = _ensemble(name)
    dZ = _dev(p['Z'])
    for k in cases.KS:
        engines[0].set_option('prune', 0)
        own = engines[0].sweep_dev('ei', p['target'], dZ.data_ptr(), len(p['Z']), k)
        for pr in (0, 1):
            got = _sweep(p, engines, p['Z'], k, pr)
            assert _same(got, own), (k, pr)
            assert got[3]['path'] == ('pruned' if pr else 'plain')
        engines[0].set_option('prune', 1)
        assert _same(engines[0].sweep_dev('ei', p['target'], dZ.data_ptr(), len(p['Z']), k), own)


def test_the_gate_under_the_default_rule():
    """prune = -1 from M = 32768 candidates and 1024 factor rows on: the result is that of prune = 0, and the gate's value is
    the mean over the members of mean(s2_m) / rho_m over its generation (any summation order of Gg positive numbers agrees
    to Gg 2^-53)."""
    name, k, m = 'se_n3_app', 10, 33001
    _, engines = _ensemble(name)
    p = cases.problem(name, m)
    Z = p['Z']
    plain = _sweep(p, engines, Z, k, 0)
    auto = _sweep(p, engines, Z, k, -1)
    assert _same(plain, auto)
    rep = auto[3]
    assert rep['path'] != 'plain' and rep['done'] == rep['Gg'] == 128 * (512 // 5)
    Gg = rep['Gg']
    want = np.mean([e.sweep('ei', p['target'], Z[:Gg], k=0, want_all=False, want_moments=True)['s2'].mean() / h[1]
                    for e, h in zip(engines, p['hypers'])])
    assert rep['gate'] == pytest.approx(want, rel=(Gg + 8) * 2.0 ** -53)
    print('gate %.4f, path %s, share %.4f' % (rep['gate'], rep['path'], auto[2]))
    assert (rep['gate'] >= 1.0 / 64) == (rep['path'] in ('pruned', 'fell back'))
    if rep['path'] == 'pruned':
        assert auto[2] == pytest.approx((Gg + cases.G + rep['nsurv']) / float(m), rel=1e-12)
        _check_bound(rep, _all_values(p, engines, Z))


def test_two_shards_merged_equal_the_whole_sweep():
    name, k = 'se_n3', 10
    _, engines = _ensemble(name)
    p = cases.problem(name, 2 * cases.M)
    whole = _sweep(p, engines, p['Z'], k, 0)
    parts = []
    for r in range(2):
        got = _sweep(p, engines, p['Z'][r * cases.M:(r + 1) * cases.M], k, 1)
        assert got[3]['path'] == 'pruned'
        parts.append((got[0], got[1] + r * cases.M))
    v = np.concatenate([q[0] for q in parts])
    i = np.concatenate([q[1] for q in parts])
    order = np.lexsort((i, -v))[:k]
    assert np.array_equal(v[order], whole[0]) and np.array_equal(i[order], whole[1])
