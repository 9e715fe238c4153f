"""Bit-exact digests of the INTERMEDIATE state of selection-only sweeps (DESIGN.md sections 2.1 to 2.3), recorded from the commit
BEFORE the single model's and the ensemble's selection steps moved into one driver, and again -- every earlier entry unchanged, the
constrained cases added -- from the commit before the multi-model sweeps got one frame: the bit-for-bit tests compare the pruned top-k
with the plain loop's, which a refactor that evaluates another set of candidates, or moves `done`, would still pass.

Per sweep: every scalar of the device's report as repr (path, M, k, G, Gg, done, cap, nsurv, tau, the gate's value, the hint flag,
... -- NaN included), the SHA-256 of ub, idx, top_val, top_idx, under prune_keep = 1 also of ub_kept, seed_idx, the dots and (where
the second bound ran) qR, ub2, idx2, and the counters sweep_trmm_launches / sweep_trmm_flop of every engine involved.

    single, prune = 1, prune_keep = 1   N = 300 (3 block rows, G = 4096), M = 13001 (off the tile grid), d = 8: SE (matrix-pipe bound by
                                        guard) and matern5 (generic bound), k = 10 and 200, each once more with prune_rows = 2
                                        (nR = min(2, nP, N / 128) = 2); the first member of ens_prune_cases' m5_n3_d5 at k = 200.
                                        All of these leave NO survivor beyond the seeds, so steps 4a-4c and launch_sel_remap do not
                                        run in them; they do at SE k = 2000 (1732 survivors, 47 after the second cut), m5_n3_d5's
                                        first member at k = 1000 (3844, 19) and its second at k = 200 (2420, then none: the empty
                                        second list) -- each asserted when recording (SURVIVORS)
    single, prune = -1                  tests/test_gpu_prune_hint.py's shape and data: f = 0.50 twice (gated and pruned, then hinted),
                                        f = 0.56 (gated, fell back), f = 1.00 (gate declined)
    ensemble, prune = 1 on the lead     se_n3 at k = 10, m5_n3_d5 at k = 200 (host form), se_n3_app at k = 10 (device form)
    ensemble, prune = -1                the hint test's three members: gated, then hinted
    illegal calls on an armed handle    UCB and a call that asks for every value, each followed by the next automatic sweep: hinted
                                        still, so the illegal call neither read nor dropped the hint (single model and ensemble)

    constrained (tests/con_cases.py)    prune = 1 on the objective: se_j2 at k = 10 and 200 (host form, each followed by the call that
                                        asks for every value and probability of feasibility: plain), m5_j3 at k = 200 (device form,
                                        1517 survivors), se_j1 with PI (not selection-legal: plain), se_j2 without an objective (plain);
                                        prune = -1: se_j2_n9 at M = 33001 twice (gated and pruned, both times)
    one lead, several entries           a forced constrained sweep, a plain ensemble sweep led by the same handle (the constrained
                                        report reads as before), a forced ensemble EI selection (it ends the constrained record)

The classes named above are asserted when recording, from the device's own report (CLASSES, CON_PATHS), so an input that drifted fails
loudly.

Output: tests/golden/select_digests.json.  Needs a GPU.  Record it from the PARENT commit's diagnostics library, never from the one
under test; tests/test_gpu_select_digests.py replays the cases:
    GPX_LIB_PATH=<parent>/pybo_amd/csrc/libgpx_diag.so python tests/golden/make_select_digests.py --commit <hash> [--out file.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, 'select_digests.json')
COUNTERS = ('sweep_trmm_launches', 'sweep_trmm_flop')

# case -> step -> (path, gate_hint) the device's report must show when recording
CLASSES = {
    'single auto f=0.50': {'sweep 1': ('pruned', False), 'sweep 2': ('pruned', True)},
    'single auto f=0.56': {'sweep 1': ('fell back', False)},
    'single auto f=1.00': {'sweep 1': ('gate declined', False)},
    'single armed, illegal calls': {'arming': ('pruned', False), 'ucb': ('plain', False), 'after ucb': ('pruned', True),
                                    'want_all': ('plain', False), 'after want_all': ('pruned', True)},
    'ensemble auto': {'sweep 1': ('pruned', False), 'sweep 2': ('pruned', True), 'ucb': ('plain', False),
                      'after ucb': ('pruned', True), 'want_all': ('plain', False), 'after want_all': ('pruned', True)},
}

# cases whose first-level survivor list must not be empty -> whether (under prune_rows = 2) the second-level list is not empty either
SURVIVORS = {
    'single forced se k=2000': True, 'single forced se k=2000 rows=2': True,
    'single forced m5_n3_d5[0] k=1000': True, 'single forced m5_n3_d5[0] k=1000 rows=2': True,
    'single forced m5_n3_d5[1] k=200 rows=2': False,
    'ensemble forced m5_n3_d5 k=200': True,
}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _record(report, top, engines, extra=()):
    """One sweep's entry: report scalars as repr, vectors as digests, the top-k pairs, every engine's counters since the last reset."""
    out = {}
    for k, v in list(report.items()) + list(extra):
        if v is None:
            continue
        if isinstance(v, np.generic):
            v = v.item()
        out[k] = _sha(v) if isinstance(v, np.ndarray) and k != 'delta' else repr(v.tolist() if isinstance(v, np.ndarray) else v)
    out['top_val'], out['top_idx'] = _sha(top[0]), _sha(top[1])
    for m, e in enumerate(engines):
        t = e.timers(reset=True)
        for c in COUNTERS:
            out['%s[%d]' % (c, m)] = repr(t[c])
    return out


def _single_sweep(e, acq, param, dZ, M, k, d_acq=None):
    e.timers(reset=True)
    top = e.sweep_dev(acq, param, dZ.data_ptr(), M, k, d_acq=d_acq)
    r = e.prune_report(vectors=True)
    extra = [('dots', e.prune_dots())] if r.get('kept') and r['path'] in ('pruned', 'fell back') else []
    return _record(r, top, [e], extra)


def _single_forced(w, k, rows):
    """prune = 1, prune_keep = 1 on the problem w (tests/test_gpu_prune.py: _small's dict)."""
    from test_gpu_prune import _dev, _fitted
    e = _fitted(w, prune=1, prune_keep=1, **({'prune_rows': rows} if rows else {}))
    target = e.mean_at_obs()[1]
    dZ = _dev(w['Xc'])
    out = {'sweep 1': _single_sweep(e, 'ei', target, dZ, len(w['Xc']), k)}
    e.close()
    return out


def _small(kernel):
    from test_gpu_prune import _small
    return _small(300, 8, 13001, seed=300, kernel=kernel)


def _member(name, i):
    """Member i of an ensemble case of tests/ens_prune_cases.py as a single model's problem."""
    import ens_prune_cases as cases
    p = cases.problem(name)
    sn2, rho, ell, bias = p['hypers'][i]
    return dict(X=p['X'], y=p['y'], ell=ell, rho=rho, sn2=sn2, bias=bias, kernel=p['kernel'], N=p['N'], d=p['d'], Xc=p['Z'])


def _single_auto(f, sweeps, illegal=False):
    """prune = -1 (the default of a fresh handle) at the hint test's shape; `illegal`: arm, then the calls that must not touch the hint."""
    import test_gpu_prune_hint as hint
    from pybo_amd._lib import Engine
    p = hint._data()
    e = Engine(0)
    target = hint._fit(e, f)
    out = {}
    if not illegal:
        for i in range(sweeps):
            out['sweep %d' % (i + 1)] = _single_sweep(e, 'ei', target, p['dZ'], hint.M, hint.K)
    else:
        out['arming'] = _single_sweep(e, 'ei', target, p['dZ'], hint.M, hint.K)
        out['ucb'] = _single_sweep(e, 'ucb', 2.0, p['dZ'], hint.M, hint.K)
        out['after ucb'] = _single_sweep(e, 'ei', target, p['dZ'], hint.M, hint.K)
        out['want_all'] = _single_sweep(e, 'ei', target, p['dZ'], hint.M, hint.K, d_acq=p['buf'].data_ptr())
        out['after want_all'] = _single_sweep(e, 'ei', target, p['dZ'], hint.M, hint.K)
    e.close()
    return out


def _ens_sweep(engines, acq, param, Z, k, want_all=False):
    from pybo_amd._lib import Engine
    for e in engines:
        e.timers(reset=True)
    r = Engine.ensemble_sweep(engines, acq, param, Z, k=k, want_all=want_all)
    return _record(Engine.ensemble_prune_report(engines, vectors=True), (r['top_val'], r['top_idx']), engines)


def _ens_forced(name, k, dev):
    """prune = 1 on the lead of the case's members (tests/test_gpu_ens_prune.py: _ensemble's construction)."""
    import ens_prune_cases as cases
    from pybo_amd._lib import Engine
    from test_gpu_ens_prune import _dev_cand
    p = cases.problem(name)
    N = p['N']
    engines = []
    for sn2, rho, ell, bias in p['hypers']:
        e = Engine(0)
        e.fit(p['X'][:N], p['y'][:N], p['kernel'], ell, rho, sn2, bias)
        for j in range(N, N + p['app']):
            assert e.append(p['X'][j], float(p['y'][j]))
        engines.append(e)
    engines[0].set_option('prune', 1)
    out = {'sweep 1': _ens_sweep(engines, 'ei', p['target'], _dev_cand(p['Z']) if dev else p['Z'], k)}
    for e in engines:
        e.close()
    return out


def _ens_auto():
    import test_gpu_prune_hint as hint
    from pybo_amd._lib import Engine
    p = hint._data()
    Z, target = p['Z'], float(np.max(p['y']))
    engines = [Engine(0) for _ in range(3)]
    for e, f in zip(engines, (0.46, 0.50, 0.54)):
        hint._fit(e, f)
    out = {}
    out['sweep 1'] = _ens_sweep(engines, 'ei', target, Z, hint.K)
    out['sweep 2'] = _ens_sweep(engines, 'ei', target, Z, hint.K)
    out['ucb'] = _ens_sweep(engines, 'ucb', 2.0, Z, hint.K)
    out['after ucb'] = _ens_sweep(engines, 'ei', target, Z, hint.K)
    out['want_all'] = _ens_sweep(engines, 'ei', target, Z, hint.K, want_all=True)
    out['after want_all'] = _ens_sweep(engines, 'ei', target, Z, hint.K)
    for e in engines:
        e.close()
    return out


def _con_engines(p):
    """[objective, constraints ..] of a problem of tests/con_cases.py, freshly fitted (tests/test_gpu_constrained.py: _fit_engines)."""
    from pybo_amd._lib import Engine
    engines = []
    for i, (sn2, rho, ell, bias) in enumerate(p['hypers']):
        e = Engine(0)
        e.fit(p['X'], p['y'] if i == 0 else p['C'][:, i - 1], p['kernel'], ell, rho, sn2, bias)
        engines.append(e)
    return engines


def _con_sweep(p, engines, acq, Z, k, obj=True, want_all=False):
    """One constrained sweep of engines[0] (obj) under engines[1:]: the lead's report, the top-k, with want_all every value and
    probability of feasibility, and the counters of the objective and of every constraint."""
    from pybo_amd._lib import Engine
    for e in engines:
        e.timers(reset=True)
    r = Engine.constrained_sweep(engines[0] if obj else None, engines[1:], p['thr'], acq, p['target'], Z, k=k, want_all=want_all,
                                 want_pof=want_all)
    lead = engines[0] if obj else engines[1]
    return _record(lead.constrained_prune_report(vectors=True), (r['top_val'], r['top_idx']), engines, [('acq', r['acq']), ('pof', r['pof'])])


def _con_forced(name, k, dev=False, acq='ei', obj=True):
    """prune = 1 on the objective of the case `name` of tests/con_cases.py; then the call that asks for every value (host form: plain)."""
    import con_cases
    from test_gpu_ens_prune import _dev_cand
    p = con_cases.problem(name)
    engines = _con_engines(p)
    engines[0].set_option('prune', 1)
    out = {'sweep 1': _con_sweep(p, engines, acq, _dev_cand(p['Z']) if dev else p['Z'], k, obj=obj)}
    if not dev:
        out['want_all'] = _con_sweep(p, engines, acq, p['Z'], k, obj=obj, want_all=True)
    for e in engines:
        e.close()
    return out


def _con_auto():
    """prune = -1 (a fresh handle's default) on se_j2_n9 at M = 33001 (Np = 1152 >= PRUNE_MIN_NP, M >= PRUNE_MIN_M and Gg + 2 G =
    13056 + 8192): two sweeps in a row.  A constrained sweep carries no decision, so both run the gate (done = Gg = 13056); it passes
    (mean s2 = 0.2365 against rho / 64) and both prune, with no survivor beyond the seeds."""
    import con_cases
    p = con_cases.problem('se_j2_n9', m=33001)
    engines = _con_engines(p)
    out = {'sweep %d' % (i + 1): _con_sweep(p, engines, 'ei', p['Z'], 10) for i in range(2)}
    for e in engines:
        e.close()
    return out


def _con_interleaved():
    """Which entry ends which of the lead's records: a plain ensemble sweep led by the objective leaves its constrained report as it
    was (the step's report IS the constrained one, read again); a forced ensemble EI selection lays the workspace out anew and ends it."""
    import con_cases
    from pybo_amd._lib import Engine, GpxError
    p = con_cases.problem('se_j2')
    engines = _con_engines(p)
    obj, pair = engines[0], engines[:2]
    obj.set_option('prune', 1)
    out = {'constrained': _con_sweep(p, engines, 'ei', p['Z'], 10)}
    for e in engines:
        e.timers(reset=True)
    r = Engine.ensemble_sweep(pair, 'ucb', 2.0, p['Z'], k=10, want_all=False)
    out['after ensemble ucb'] = _record(obj.constrained_prune_report(vectors=True), (r['top_val'], r['top_idx']), engines)
    r = Engine.ensemble_sweep(pair, 'ei', p['target'], p['Z'], k=10, want_all=False)
    out['ensemble ei'] = _record(Engine.ensemble_prune_report(pair, vectors=True), (r['top_val'], r['top_idx']), engines)
    try:
        obj.constrained_prune_report()
        code = 0
    except GpxError as err:
        code = err.code
    out['ensemble ei']['constrained report'] = repr(code)
    for e in engines:
        e.close()
    return out


# constrained case -> step -> the path the lead's report must show when recording (a constrained report has no gate_hint)
CON_PATHS = {
    'constrained forced se_j2 k=10': {'sweep 1': 'pruned', 'want_all': 'plain'},
    'constrained forced se_j2 k=200': {'sweep 1': 'pruned', 'want_all': 'plain'},
    'constrained forced m5_j3 k=200 dev': {'sweep 1': 'pruned'},
    'constrained pi se_j1 k=10': {'sweep 1': 'plain', 'want_all': 'plain'},
    'constrained no objective se_j2 k=10': {'sweep 1': 'plain', 'want_all': 'plain'},
    'constrained auto se_j2_n9': {'sweep 1': 'pruned', 'sweep 2': 'pruned'},
    'constrained interleaved': {'constrained': 'pruned', 'after ensemble ucb': 'pruned', 'ensemble ei': 'pruned'},
}


def con_cases_list():
    out = [('constrained forced se_j2 k=%d' % k, lambda k=k: _con_forced('se_j2', k)) for k in (10, 200)]
    out.append(('constrained forced m5_j3 k=200 dev', lambda: _con_forced('m5_j3', 200, dev=True)))
    out.append(('constrained pi se_j1 k=10', lambda: _con_forced('se_j1', 10, acq='pi')))
    out.append(('constrained no objective se_j2 k=10', lambda: _con_forced('se_j2', 10, obj=False)))
    out.append(('constrained auto se_j2_n9', _con_auto))
    out.append(('constrained interleaved', _con_interleaved))
    return out


def cases():
    """[(name, thunk)]: every thunk returns {step: {output: repr or digest}}."""
    out = []
    for kernel in ('se', 'matern5'):
        for k in (10, 200):
            for rows in (0, 2):
                out.append(('single forced %s k=%d%s' % (kernel, k, ' rows=2' if rows else ''),
                            lambda kernel=kernel, k=k, rows=rows: _single_forced(_small(kernel), k, rows)))
    # survivor lists that are not empty (SURVIVORS: asserted when recording); m5_n3_d5's first member alone leaves none at k = 200 --
    # recorded all the same -- but 3844 at k = 1000 (19 after the second cut), its second member 2420 at k = 200 (none after it)
    for rows in (0, 2):
        tag = ' rows=2' if rows else ''
        out.append(('single forced se k=2000' + tag, lambda rows=rows: _single_forced(_small('se'), 2000, rows)))
        out.append(('single forced m5_n3_d5[0] k=200' + tag, lambda rows=rows: _single_forced(_member('m5_n3_d5', 0), 200, rows)))
        out.append(('single forced m5_n3_d5[0] k=1000' + tag, lambda rows=rows: _single_forced(_member('m5_n3_d5', 0), 1000, rows)))
    out.append(('single forced m5_n3_d5[1] k=200 rows=2', lambda: _single_forced(_member('m5_n3_d5', 1), 200, 2)))
    out.append(('single auto f=0.50', lambda: _single_auto(0.50, 2)))
    out.append(('single auto f=0.56', lambda: _single_auto(0.56, 1)))
    out.append(('single auto f=1.00', lambda: _single_auto(1.00, 1)))
    out.append(('single armed, illegal calls', lambda: _single_auto(0.50, 0, illegal=True)))
    out.append(('ensemble forced se_n3 k=10', lambda: _ens_forced('se_n3', 10, False)))
    out.append(('ensemble forced m5_n3_d5 k=200', lambda: _ens_forced('m5_n3_d5', 200, False)))
    out.append(('ensemble forced se_n3_app k=10 dev', lambda: _ens_forced('se_n3_app', 10, True)))
    out.append(('ensemble auto', _ens_auto))
    return out + con_cases_list()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit the loaded library was built from')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    from pybo_amd import _lib
    doc = dict(commit=args.commit, library=os.path.basename(_lib.LIB_PATH), cases={})
    for name, run in cases():
        first, second = run(), run()
        # an output the recording library does not reproduce run to run is left out (and named on stderr): a finding about it
        unstable = sorted('%s / %s' % (s, k) for s in first for k in first[s] if second[s].get(k) != first[s][k])
        if unstable:
            print('NOT reproducible in %s: %s' % (name, unstable), file=sys.stderr)
            first = {s: {k: v for k, v in first[s].items() if second[s].get(k) == v} for s in first}
        for step, (path, hinted) in CLASSES.get(name, {}).items():
            assert (first[step]['path'], first[step]['gate_hint']) == (repr(path), repr(hinted)), (name, step, first[step])
        for step, path in CON_PATHS.get(name, {}).items():
            assert first[step]['path'] == repr(path), (name, step, first[step])
        if name == 'constrained interleaved':      # the second reading of the constrained report is the first; the forced ensemble sweep ends it
            a, b = first['constrained'], first['after ensemble ucb']
            assert all(b[k] == a[k] for k in a if not k.startswith(('top_', 'sweep_trmm_'))), (a, b)
            assert first['ensemble ei']['constrained report'] == repr(-5), first['ensemble ei']
        if name.startswith(('single forced', 'ensemble forced')):
            assert first['sweep 1']['path'] == repr('pruned'), (name, first['sweep 1'])
        if name in SURVIVORS:
            assert int(first['sweep 1']['nsurv']) > 0, (name, first['sweep 1'])
            if name.endswith('rows=2'):          # steps 4a-4c ran; the second list is empty exactly where SURVIVORS says so
                assert first['sweep 1']['nR'] == '2' and 'idx2' in first['sweep 1'], (name, first['sweep 1'])
                assert (int(first['sweep 1']['nsurv2']) > 0) == SURVIVORS[name], (name, first['sweep 1'])
        doc['cases'][name] = first
        print(name, 'ok:', {s: '%s nsurv %s done %s nR %s' % (r['path'], r['nsurv'], r['done'], r.get('nR')) for s, r in first.items()},
              flush=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s (%d cases)' % (args.out, len(doc['cases'])))


if __name__ == '__main__':
    main()
