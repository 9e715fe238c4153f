"""The gate's decision carried from one selection-only sweep to the next (pybo_amd/csrc/prune_hint.h, DESIGN.md section 2.1 step 1 and
section 2.2 step 1): under option "prune" = -1 a sweep that pruned and left at most cap / 2 first-level survivors lets the next sweep
of the same shape on the handle skip the gate's exact generation (done = 0, as "prune" = 1).  The decision survives fits, is dropped
by any option call, by another shape, by a sweep that did not earn it and by a declined gate, and never changes a result: every
top-k here is array_equal to the plain loop's.

The smallest shape the automatic rule accepts: N = 1024 (nP = 8, G = 4096, Gg = 16384), M = 40961 (cap = 10240), d = 8, SE-ARD,
k = 10; the second bound never runs at nP < 32, so a pruned sweep's flop are N^2 (done + G + nsurv).  Length scales f * ones(d), with
the classes the CPU oracle gives (gate = mean(s2[:Gg]) / rho; nsurv gated / hinted):
    f = 0.50   gate 0.0615   2710 / 0       pruned, arms
    f = 0.53   gate 0.0430   6596 / 1845    gated: pruned but in (cap / 2, cap], does not arm;  hinted: stays armed
    f = 0.56   gate 0.0302   12645 / 5034   gated: fell back
    f = 1.00   gate 0.00057  - / 34770      the gate declines;  a stale hint falls back
Every test asserts the class it is there for from the device's own report, so an input that drifted out of its class fails loudly.

The plain loop's result is taken by a prune = 0 sweep before "prune" is set to -1 (once); where a reference is needed later, on a
handle whose hint must live on, by the call that also asks for every value: it never prunes, runs the plain loop's launches and
makes no option call (shown equal to the prune = 0 sweep in `_armed`)."""
import numpy as np
import pytest

from test_gpu_prune import _DevBuf, _dev

pytestmark = pytest.mark.gpu

N, D, M, K = 1024, 8, 40961, 10
G, GG, CAP = 4096, 16384, 10240

_DATA = {}


def _data():
    if not _DATA:
        rng = np.random.RandomState(2)
        X = rng.rand(N, D)
        y = -np.sum((X - 0.5) ** 2, axis=1) + 1e-3 * rng.randn(N)
        Z = np.random.RandomState(5).rand(M, D)
        _DATA.update(X=X, y=y, rho=float(np.var(y)), bias=float(np.mean(y)), Z=Z, dZ=_dev(Z), buf=_DevBuf(M))
    return _DATA


def _fit(e, f):
    """(Re)fit e with length scales f * ones(d); returns the EI target, the largest posterior mean at the observations."""
    p = _data()
    e.fit(p['X'], p['y'], 'se', f * np.ones(D), p['rho'], 1e-4 * p['rho'], p['bias'])
    return e.mean_at_obs()[1]


def _plain(e, target, m=M, k=K):
    """The plain loop's top-k without an option call: the call that also returns every value never prunes."""
    p = _data()
    got = e.sweep_dev('ei', target, p['dZ'].data_ptr(), m, k, d_acq=p['buf'].data_ptr())
    assert e.prune_report(vectors=False)['path'] == 'plain'
    return got


def _sweep(e, target, m=M, k=K):
    """One selection-only sweep: (top_val, top_idx), its report, its timers."""
    e.timers(reset=True)
    got = e.sweep_dev('ei', target, _data()['dZ'].data_ptr(), m, k)
    t = e.timers(reset=True)
    r = e.prune_report(vectors=False)
    r['share'] = t['sweep_trmm_flop'] / (float(N) ** 2 * m)
    print('M %d k %d: %s, hint %s, done %d, gate %.4g, nsurv %d, share %.4f, launches %d' %
          (m, k, r['path'], r['gate_hint'], r['done'], r['gate_s2'] / _data()['rho'], r['nsurv'], r['share'], t['sweep_trmm_launches']))
    return got, r, t


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _gated(r, gate='gate_s2'):
    """The gate ran (the report's `done` is the bound pass's: a declined gate leaves it 0)."""
    return not r['gate_hint'] and np.isfinite(r[gate]) and r['done'] == (0 if r['path'] == 'gate declined' else GG)


def _hinted(r, gate='gate_s2'):
    return r['gate_hint'] and r['done'] == 0 and np.isnan(r[gate]) and r['path'] in ('pruned', 'fell back')


def _start(f):
    """A fresh handle fitted at f: (engine, target, the prune = 0 result); "prune" is -1 from here on."""
    from pybo_amd._lib import Engine
    e = Engine(0)
    target = _fit(e, f)
    e.set_option('prune', 0)
    plain = e.sweep_dev('ei', target, _data()['dZ'].data_ptr(), M, K)
    assert e.prune_report(vectors=False)['path'] == 'plain'
    assert _same(plain, _plain(e, target))                # the two forms of the reference
    e.set_option('prune', -1)
    return e, target, plain


def _armed():
    """f = 0.50: the gated sweep that arms, then the hinted one."""
    e, target, plain = _start(0.50)
    s1 = _sweep(e, target)
    s2 = _sweep(e, target)
    assert _same(s1[0], plain) and _same(s2[0], plain)
    assert s1[1]['path'] == 'pruned' and _gated(s1[1]) and s1[1]['nsurv'] <= CAP // 2
    assert s2[1]['path'] == 'pruned' and _hinted(s2[1]) and s2[1]['nsurv'] <= CAP // 2
    return e, target, plain, s1, s2


def test_a_sweep_that_paid_arms_the_hint_and_the_next_one_skips_the_gate():
    e, target, plain, s1, s2 = _armed()
    chunk = (M + 127) // 128 * 128                         # one chunk holds every launch of this shape
    for _, r, t in (s1, s2):
        assert (r['M'], r['k'], r['G'], r['Gg'], r['cap'], r['nR']) == (M, K, G, GG, CAP, 0)
        assert t['sweep_trmm_flop'] == float(N) ** 2 * (r['done'] + G + r['nsurv'])
        # the gate's launch (where it ran), the seeds', the survivors'
        assert t['sweep_trmm_launches'] == (r['done'] > 0) + 1 + (r['nsurv'] + chunk - 1) // chunk
    # the gate's launch is gone: what is left differs only by the survivors' chain
    surv_launches = [(r['nsurv'] + chunk - 1) // chunk for _, r, _ in (s1, s2)]
    assert (s1[2]['sweep_trmm_launches'] - surv_launches[0]) - (s2[2]['sweep_trmm_launches'] - surv_launches[1]) == 1
    e.close()


def test_the_hint_survives_a_refit():
    e = _armed()[0]
    target = _fit(e, 0.53)
    want = _plain(e, target)
    got, r, _ = _sweep(e, target)
    assert _same(got, want) and r['path'] == 'pruned' and _hinted(r) and r['nsurv'] <= CAP // 2
    got, r, _ = _sweep(e, target)
    assert _same(got, want) and r['path'] == 'pruned' and _hinted(r)
    e.close()


def test_an_option_call_drops_the_hint():
    e, target, plain = _armed()[:3]
    e.set_option('prune', -1)
    got, r, _ = _sweep(e, target)
    assert _same(got, plain) and r['path'] == 'pruned' and _gated(r)
    got, r, _ = _sweep(e, target)                          # ... and that sweep armed it again
    assert _same(got, plain) and _hinted(r)
    with pytest.raises(Exception):
        e.set_option('no_such_option', 1)                  # a refused call drops it too
    got, r, _ = _sweep(e, target)
    assert _same(got, plain) and _gated(r)
    e.close()


def test_another_candidate_count_or_another_k_drops_the_hint():
    e, target, plain = _armed()[:3]
    m = 36000
    got, r, _ = _sweep(e, target, m=m)
    assert _same(got, _plain(e, target, m=m)) and r['M'] == m and _gated(r)
    got, r, _ = _sweep(e, target)                          # back: the key is the smaller set's by now
    assert _same(got, plain) and _gated(r) and r['path'] == 'pruned' and r['nsurv'] <= CAP // 2
    got, r, _ = _sweep(e, target)
    assert _same(got, plain) and _hinted(r)
    got, r, _ = _sweep(e, target, k=K + 1)
    assert _same(got, _plain(e, target, k=K + 1)) and r['k'] == K + 1 and _gated(r)
    e.close()


def test_a_pruned_sweep_above_half_the_fallback_line_does_not_arm():
    e, target, plain = _start(0.53)
    for _ in range(2):
        got, r, _ = _sweep(e, target)
        assert _same(got, plain) and r['path'] == 'pruned' and _gated(r)
        assert CAP // 2 < r['nsurv'] <= CAP
    e.close()


def test_a_sweep_that_fell_back_does_not_arm():
    e, target, plain = _start(0.56)
    for _ in range(2):
        got, r, _ = _sweep(e, target)
        assert _same(got, plain) and r['path'] == 'fell back' and _gated(r)
        assert r['nsurv'] > CAP
    e.close()


def test_a_stale_hint_costs_one_fallback_and_the_gate_is_back():
    e = _armed()[0]
    target = _fit(e, 1.00)
    want = _plain(e, target)
    got, r, t = _sweep(e, target)
    assert _same(got, want) and r['path'] == 'fell back' and _hinted(r) and r['nsurv'] > CAP
    assert r['share'] >= 1.0 and t['sweep_trmm_flop'] == float(N) ** 2 * (G + M)      # the seeds, then the plain loop from 0
    got, r, _ = _sweep(e, target)
    assert _same(got, want) and r['path'] == 'gate declined' and _gated(r) and r['share'] == 1.0
    assert r['gate_s2'] < _data()['rho'] / 64.0
    e.close()


def test_no_hint_is_armed_where_the_gate_declines():
    e, target, plain = _start(1.00)
    for _ in range(2):
        got, r, t = _sweep(e, target)
        assert _same(got, plain) and r['path'] == 'gate declined' and _gated(r)
        assert r['share'] == 1.0 and t['sweep_bound'] == 0.0
    e.close()


def test_the_ensemble_sweep_carries_its_gate_decision_on_the_lead():
    from pybo_amd._lib import Engine
    p = _data()
    Z, target = p['Z'], float(np.max(p['y']))
    engines = [Engine(0) for _ in range(3)]

    def fit(fs):
        for e, f in zip(engines, fs):
            _fit(e, f)

    def plain():
        """No option call: the call that also returns every value never prunes."""
        r = Engine.ensemble_sweep(engines, 'ei', target, Z, k=K, want_all=True)
        assert Engine.ensemble_prune_report(engines, vectors=False)['path'] == 'plain'
        return r['top_val'], r['top_idx']

    def sweep():
        r = Engine.ensemble_sweep(engines, 'ei', target, Z, k=K, want_all=False)
        rep = Engine.ensemble_prune_report(engines, vectors=False)
        print('ensemble: %s, hint %s, done %d, gate %.4g, nsurv %d' % (rep['path'], rep['gate_hint'], rep['done'], rep['gate'], rep['nsurv']))
        assert (rep['M'], rep['k'], rep['G'], rep['Gg'], rep['cap']) == (M, K, G, GG, CAP)
        return (r['top_val'], r['top_idx']), rep

    def gated(rep):
        return _gated(rep, 'gate')

    def hinted(rep):
        return _hinted(rep, 'gate')

    fit((0.46, 0.50, 0.54))
    engines[0].set_option('prune', 0)
    r = Engine.ensemble_sweep(engines, 'ei', target, Z, k=K, want_all=False)
    want = (r['top_val'], r['top_idx'])
    assert Engine.ensemble_prune_report(engines, vectors=False)['path'] == 'plain'
    assert _same(want, plain())
    engines[0].set_option('prune', -1)
    got, rep = sweep()
    assert _same(got, want) and rep['path'] == 'pruned' and gated(rep) and rep['nsurv'] <= CAP // 2
    got, rep = sweep()
    assert _same(got, want) and rep['path'] == 'pruned' and hinted(rep) and rep['nsurv'] <= CAP // 2
    engines[1].set_option('prune', -1)                      # a member's options are its own: the lead's hint lives on
    got, rep = sweep()
    assert _same(got, want) and hinted(rep)
    engines[0].set_option('prune', -1)
    got, rep = sweep()
    assert _same(got, want) and rep['path'] == 'pruned' and gated(rep) and rep['nsurv'] <= CAP // 2
    # refitted members: the armed hint is used, the result is the plain loop's, and the hint is what this sweep earned
    fit((0.9, 1.0, 1.1))
    want = plain()
    got, rep = sweep()
    assert _same(got, want) and hinted(rep) and rep['path'] in ('pruned', 'fell back')
    earned = rep['path'] == 'pruned' and rep['nsurv'] <= CAP // 2
    got, rep = sweep()
    assert _same(got, want) and rep['gate_hint'] == earned and (hinted(rep) if earned else gated(rep))
    for e in engines:
        e.close()
