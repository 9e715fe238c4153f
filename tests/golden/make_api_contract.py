"""The host-side contract of the C-ABI: what gpx_set_option, GPX_OPTIONS and the sweep wrappers answer to values and
arguments at and beyond every boundary, for the shipping library (libgpx.so) and the diagnostics build (libgpx_diag.so).

    gpx_set_option   every option name of the library and a few unknown ones, for each value of VALUES: (rc, message)
    GPX_OPTIONS      gpx_create under each string of ENV_OPTIONS: (rc, gpx_last_error(NULL) when rc != 0)
    wrappers         one call per single bad argument of gpx_sweep(_dev), gpx_sweep_update(_dev), gpx_ensemble_sweep(_dev)
                     (two members), gpx_rff_gram_batch, gpx_rff_posterior, gpx_constrained_sweep(_dev), gpx_ehvi_sweep(_dev),
                     gpx_ehvi_fold_dev, gpx_sweep_batch, gpx_sweep_batch_fantasy, gpx_ensemble_sweep_batch and gpx_path_sweep(_dev), on handles fitted to
                     N = 10, d = 2: (rc, message)

None of the recorded calls reaches a HIP runtime error, so no message carries a source line.  Output:
tests/golden/api_contract.json (messages stored once, results as [rc, message index or -1]).  Needs a GPU; recorded from
the libraries of the commit before the option table replaced gpx_set_option's if-chain, recorded again with the rows of the
constrained, two-objective, batch and pathwise entries from the commit before those entries got one frame (every earlier row came
out unchanged), once more with the rows of gpx_sweep_batch_fantasy from the commit before the batch entries got one driver (again
every earlier row unchanged), and replayed against the current ones by tests/test_gpu_api_contract.py:
    python tests/golden/make_api_contract.py [--ship path/libgpx.so] [--diag path/libgpx_diag.so] [--out file.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pybo_amd import _lib                   # noqa: E402  (the prototypes only; the libraries are loaded by path)

OUT = os.path.join(HERE, 'api_contract.json')
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
VALUES = [-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 127, 128, 129, 255, 256, 65535, 65536, 65537,
          131072, 100000, 100001, 10 ** 6, 10 ** 6 + 1, 10 ** 7, 10 ** 7 + 1, 10 ** 9, 10 ** 9 + 1, 2 ** 31, -2 ** 31 - 1,
          I64_MIN, I64_MAX]
# every option gpx_set_option knew before the table, then names it must not know ("prune" and "prune_keep" came after it:
# tests/test_abi.py::test_option_table_agrees_with_the_headers covers every row of the table, those two included)
OPTIONS = ['chunk', 'super_m', 'tile_order', 'sweep_cache', 'chol_w', 'chol_tg', 'chol_tg_chunks', 'chol_tg_grid',
           'chol_tg_trace', 'chol_tg_tmo_ms', 'chol_tg_min', 'chol_tg_max', 'chol_tg_isolate', 'chol_tg_nap', 'chol_tg_db',
           'chol_tg_db_max', 'chol_tg_fuse', 'trtri_ahead', 'trtri_ahead_min', 'chol_fuse', 'chol_graph', 'chol_merge',
           'chol_rl', 'x_skip', 'x_bg', 'x_bg_lds', 'x_bg_iters', 'x_rff', 'grad_form', 'grad_rb_cs', 'grad_kernel',
           'trtri_left', 'refine_inverse', 'eager_inverse']
UNKNOWN = ['', 'CHUNK', 'chunk ', 'chol', 'chol_tg_', 'chol_tg_foo', 'chol_tgx', 'trtri_ahead_', 'trtri_aheadx', 'x_bg_',
           'x_bgl', 'x_bg_l', 'x_rff2', 'sweep_cache=1']
ENV_OPTIONS = ['chunk=256', 'chunk=256,tile_order=27,chol_tg=0', 'bogus=1', 'chunk=100', 'chunk', '=5', 'chunk=256,',
               ',,chunk=256,,', 'chunk=abc', 'chunk=12x', 'chunk=', 'chunk= 256', 'x_skip=1', 'chol_tg=2,chunk=256']


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in list(_lib.SYMBOLS.items()) + list(_lib.DIAG_SYMBOLS.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _err(lib, h, rc):
    return [rc, lib.gpx_last_error(h).decode() if rc != 0 else None]


def probe(path):
    """{case: [rc, message or None]} (option cases: a list over VALUES) for the library at `path`."""
    lib = load(path)
    out = {}

    def handle():
        h = C.c_void_p()
        assert lib.gpx_create(0, None, C.byref(h)) == 0, lib.gpx_last_error(None)
        return h

    # -- gpx_set_option on a handle of its own (x_rff is process-wide: set back to 0 at the end)
    h = handle()
    for name in OPTIONS + UNKNOWN:
        out['set_option %r' % name] = [_err(lib, h, lib.gpx_set_option(h, name.encode(), v)) for v in VALUES]
    lib.gpx_set_option(h, b'x_rff', 0)
    before = lib.gpx_last_error(h)
    out['set_option NULL name'] = [lib.gpx_set_option(h, None, 1), None, lib.gpx_last_error(h) == before]   # message untouched
    out['set_option NULL handle'] = [lib.gpx_set_option(None, b'chunk', 256), None]
    lib.gpx_destroy(h)

    # -- GPX_OPTIONS
    saved = os.environ.pop('GPX_OPTIONS', None)
    try:
        for s in ENV_OPTIONS:
            os.environ['GPX_OPTIONS'] = s
            g = C.c_void_p()
            rc = lib.gpx_create(0, None, C.byref(g))
            out['GPX_OPTIONS %r' % s] = [rc, lib.gpx_last_error(None).decode() if rc != 0 else None, bool(g.value)]
            if g.value:
                lib.gpx_destroy(g)
    finally:
        os.environ.pop('GPX_OPTIONS', None)
        if saved is not None:
            os.environ['GPX_OPTIONS'] = saved

    # -- the wrappers, on models fitted to N = 10, d = 2 (a third member with d = 3 for the ensemble's shape check)
    rng = np.random.RandomState(7)
    M, d = 64, 2
    X, y = rng.rand(10, d), rng.rand(10)
    Xc = rng.rand(M, d)
    prm = np.array([0.5])
    tv, ti = np.zeros(8), np.zeros(8, dtype=np.int64)
    acq, mu, s2 = np.zeros(M), np.zeros(M), np.zeros(M)
    unfit, a, b, c = handle(), handle(), handle(), handle()
    for hh, Xh in ((a, X), (b, X), (c, rng.rand(10, 3))):
        rc = lib.gpx_fit(hh, _p(Xh), 10, Xh.shape[1], _p(y), 0, _p(np.full(Xh.shape[1], 0.4)), 1.0, 1e-3, 0.0)
        assert rc == 0, lib.gpx_last_error(hh)
    grid = C.c_void_p()
    assert lib.gpx_grid_create(0, 0, _p(np.array([0.0, 1.0] * d)), M, d, 3, 0, None, 0, C.byref(grid)) == 0
    dXc = lib.gpx_grid_data(grid)

    # single bad arguments (and pairs that show which check fires first) of a sweep: (acq, params, nparams, M, k, tv, ti)
    good = dict(acq=0, prm=prm, np_=1, M=M, k=5, tv=tv, ti=ti)
    bad = [('not fitted', dict(h='unfit')), ('acq -1', dict(acq=-1)), ('acq 4', dict(acq=4)), ('nparams 0', dict(np_=0)),
           ('params NULL', dict(prm=None)), ('k -1', dict(k=-1)), ('k 4097', dict(k=4097)), ('top_val NULL', dict(tv=None)),
           ('top_idx NULL', dict(ti=None)), ('acq 4 + k -1', dict(acq=4, k=-1)), ('nparams 0 + k 4097', dict(np_=0, k=4097)),
           ('k -1 + top_val NULL', dict(k=-1, tv=None)), ('M 0', dict(M=0)), ('M 0 + acq 4', dict(M=0, acq=4)),
           ('mean, no params', dict(acq=3, prm=None, np_=0, k=0)), ('ok', {})]
    for form in ('host', 'dev'):
        for label, kw in bad:
            a_ = dict(good, **kw)
            hh = unfit if kw.get('h') == 'unfit' else a
            if form == 'host':
                rc = lib.gpx_sweep(hh, a_['acq'], _p(a_['prm']), a_['np_'], _p(Xc), a_['M'], a_['k'], _p(a_['tv']), _p(a_['ti']),
                                   _p(acq), _p(mu), _p(s2))
            else:
                rc = lib.gpx_sweep_dev(hh, a_['acq'], _p(a_['prm']), a_['np_'], dXc, a_['M'], a_['k'], _p(a_['tv']), _p(a_['ti']),
                                       None, None, None)
            out['sweep %s: %s' % (form, label)] = _err(lib, hh, rc)
        out['sweep %s: Xc NULL' % form] = _err(lib, a, lib.gpx_sweep(a, 0, _p(prm), 1, None, M, 5, _p(tv), _p(ti), None, None, None)
                                               if form == 'host' else
                                               lib.gpx_sweep_dev(a, 0, _p(prm), 1, None, M, 5, _p(tv), _p(ti), None, None, None))

    def update(form, hh, a_):
        if form == 'host':
            return lib.gpx_sweep_update(hh, a_['acq'], _p(a_['prm']), a_['np_'], a_['k'], _p(a_['tv']), _p(a_['ti']),
                                        _p(acq), _p(mu), _p(s2))
        return lib.gpx_sweep_update_dev(hh, a_['acq'], _p(a_['prm']), a_['np_'], a_['k'], _p(a_['tv']), _p(a_['ti']),
                                        None, None, None)

    for form in ('host', 'dev'):                   # no cache yet
        out['sweep_update %s: no cache' % form] = _err(lib, a, update(form, a, good))
        out['sweep_update %s: not fitted' % form] = _err(lib, unfit, update(form, unfit, good))
    assert lib.gpx_set_option(a, b'sweep_cache', 1) == 0
    assert lib.gpx_sweep(a, 0, _p(prm), 1, _p(Xc), M, 5, _p(tv), _p(ti), None, None, None) == 0
    for form in ('host', 'dev'):
        for label, kw in bad:
            if 'M' in kw or kw.get('h'):
                continue
            out['sweep_update %s: %s' % (form, label)] = _err(lib, a, update(form, a, dict(good, **kw)))

    def ens(form, mem, n, a_, X_=True, moments=False):
        arr = (C.c_void_p * max(len(mem), 1))(*[m.value if m is not None else None for m in mem])
        if form == 'host':
            return lib.gpx_ensemble_sweep(arr if mem else None, n, a_['acq'], _p(a_['prm']), a_['np_'], _p(Xc) if X_ else None,
                                          a_['M'], a_['k'], _p(a_['tv']), _p(a_['ti']), _p(acq),
                                          _p(mu) if moments else None, _p(s2) if moments else None)
        return lib.gpx_ensemble_sweep_dev(arr if mem else None, n, a_['acq'], _p(a_['prm']), a_['np_'], dXc if X_ else None,
                                          a_['M'], a_['k'], _p(a_['tv']), _p(a_['ti']), None, None, None)

    for form in ('host', 'dev'):
        for label, kw in bad:
            if kw.get('h'):
                continue
            out['ensemble %s: %s' % (form, label)] = _err(lib, a, ens(form, [a, b], 2, dict(good, **kw)))
        out['ensemble %s: Xc NULL' % form] = _err(lib, a, ens(form, [a, b], 2, good, X_=False))
        out['ensemble %s: Xc NULL + acq 4' % form] = _err(lib, a, ens(form, [a, b], 2, dict(good, acq=4), X_=False))
        if form == 'host':                        # (only the host form checks the moments; no host buffer goes to a _dev form)
            out['ensemble host: moments with EI'] = _err(lib, a, ens(form, [a, b], 2, good, moments=True))
            out['ensemble host: moments with EI + acq 4'] = _err(lib, a, ens(form, [a, b], 2, dict(good, acq=4), moments=True))
        out['ensemble %s: member not fitted' % form] = _err(lib, a, ens(form, [a, unfit], 2, good))
        out['ensemble %s: member d 3' % form] = _err(lib, a, ens(form, [a, c], 2, good))
        out['ensemble %s: member NULL' % form] = _err(lib, a, ens(form, [a, None], 2, good))
        out['ensemble %s: members NULL' % form] = [ens(form, [], 2, good), None]
        out['ensemble %s: n 0' % form] = [ens(form, [a, b], 0, good), None]

    # the RFF wrappers whose wide-feature paths share the per-draw upload (n = 128: the wide path)
    n = 128
    W, bb, z = rng.randn(2 * n * d), rng.rand(2 * n), rng.randn(2 * n)
    A, v, th = np.zeros(2 * n * n), np.zeros(2 * n), np.zeros(2 * n)
    for label, hh, args in (('not fitted', unfit, (W, bb, 2, n)), ('W NULL', a, (None, bb, 2, n)), ('b NULL', a, (W, None, 2, n)),
                            ('S 0', a, (W, bb, 0, n)), ('n 0', a, (W, bb, 2, 0))):
        Wp, bp, S_, n_ = args
        out['rff_gram_batch: %s' % label] = _err(lib, hh, lib.gpx_rff_gram_batch(hh, _p(Wp), _p(bp), S_, n_, _p(A), _p(v)))
    out['rff_gram_batch: A NULL'] = _err(lib, a, lib.gpx_rff_gram_batch(a, _p(W), _p(bb), 2, n, None, _p(v)))
    for label, hh, args in (('not fitted', unfit, (W, bb, z, 2, n, 1.0)), ('z NULL', a, (W, bb, None, 2, n, 1.0)),
                            ('W NULL', a, (None, bb, z, 2, n, 1.0)), ('n 4097', a, (W, bb, z, 2, 4097, 1.0)),
                            ('sc 0', a, (W, bb, z, 2, n, 0.0)), ('sc NaN', a, (W, bb, z, 2, n, float('nan'))),
                            ('S 0', a, (W, bb, z, 0, n, 1.0))):
        Wp, bp, zp, S_, n_, sc = args
        out['rff_posterior: %s' % label] = _err(lib, hh, lib.gpx_rff_posterior(hh, _p(Wp), _p(bp), _p(zp), S_, n_, sc, _p(th)))
    out['rff_posterior: theta NULL'] = _err(lib, a, lib.gpx_rff_posterior(a, _p(W), _p(bb), _p(z), 2, n, 1.0, None))

    # -- the entries that drive several handles from one lead, the batch entries and the pathwise sweep: refusals only (one bad argument
    #    per call, then pairs that show which check fires first).  `a` holds a live sweep cache of M candidates from here on, `b` none yet.
    def arr(hs):
        return (C.c_void_p * max(len(hs), 1))(*[x.value if x is not None else None for x in hs])

    nan, inf = float('nan'), float('inf')
    thr2 = np.array([0.1, 0.2])
    cgood = dict(obj=a, cons=[b], thr=np.array([0.1]), acq=0, prm=prm, np_=1, X=True, M=M, k=5, tv=tv, ti=ti)
    cbad = [('nc 0', dict(cons=[])), ('cons NULL', dict(cons=None, nc=1)), ('nc 17', dict(cons=[b] * 17, thr=np.zeros(17))),
            ('constraint NULL', dict(cons=[b, None], thr=thr2)), ('thr NULL', dict(thr=None)), ('thr inf', dict(cons=[b, c], thr=np.array([0.0, inf]))),
            ('thr NaN', dict(thr=np.array([nan]))), ('acq ucb', dict(acq=2)), ('acq mean', dict(acq=3, prm=None, np_=0)),
            ('acq mes', dict(acq=16, prm=np.array([0.5, 0.6]), np_=2)), ('acq kg', dict(acq=32, prm=Xc[:2].ravel().copy(), np_=4)),
            ('acq 4', dict(acq=4)), ('params NULL', dict(prm=None, np_=0)), ('M 0', dict(M=0)), ('Xc NULL', dict(X=False)),
            ('no objective, M 0', dict(obj=None, M=0)), ('k 4097', dict(k=4097)), ('k -1', dict(k=-1)), ('top_val NULL', dict(tv=None)),
            ('twice', dict(cons=[b, b], thr=thr2)), ('objective twice', dict(cons=[b, a], thr=thr2)),
            ('no objective, twice', dict(obj=None, cons=[a, b, a], thr=np.zeros(3))), ('constraint not fitted', dict(cons=[b, unfit], thr=thr2)),
            ('objective not fitted', dict(obj=unfit)), ('constraint d 3', dict(cons=[b, c], thr=thr2)),
            ('no objective, acq ucb unread', dict(obj=None, acq=2, M=0)),
            ('nc 17 + thr NULL', dict(cons=[b] * 17, thr=None)), ('constraint NULL + thr NULL', dict(cons=[b, None], thr=None)),
            ('thr NaN + acq ucb', dict(thr=np.array([nan]), acq=2)), ('acq ucb + params NULL', dict(acq=2, prm=None, np_=0)),
            ('params NULL + M 0', dict(prm=None, np_=0, M=0)), ('M 0 + k 4097', dict(M=0, k=4097)), ('k 4097 + twice', dict(k=4097, cons=[b, b], thr=thr2)),
            ('twice + not fitted', dict(cons=[unfit, unfit], thr=thr2)), ('objective not fitted + constraint d 3', dict(obj=unfit, cons=[c])),
            ('constraint not fitted + d 3', dict(cons=[c, unfit], thr=thr2))]
    for form in ('host', 'dev'):
        fn = lib.gpx_constrained_sweep if form == 'host' else lib.gpx_constrained_sweep_dev
        for label, kw in cbad:
            g_ = dict(cgood, **kw)
            lead = g_['obj'] if g_['obj'] is not None else g_['cons'][0]
            Xp = None if not g_['X'] else (_p(Xc) if form == 'host' else dXc)
            rc = fn(g_['obj'], arr(g_['cons']) if g_['cons'] is not None else None, g_.get('nc', len(g_['cons'] or ())), _p(g_['thr']), g_['acq'], _p(g_['prm']),
                    g_['np_'], Xp, g_['M'], g_['k'], _p(g_['tv']), _p(g_['ti']), None, None)
            out['constrained %s: %s' % (form, label)] = _err(lib, lead, rc)
        out['constrained %s: no handle' % form] = [fn(None, None, 0, _p(thr2), 0, _p(prm), 1, _p(Xc) if form == 'host' else dXc, M, 5, _p(tv), _p(ti),
                                                      None, None), None]

    front, ref = np.array([0.3, 0.1, 0.1, 0.3]), np.array([0.0, 0.0])
    egood = dict(f1=a, f2=b, P=front, np_=2, ref=ref, X=True, M=M, k=5, tv=tv, ti=ti)
    ebad = [('f2 NULL', dict(f2=None)), ('f1 == f2', dict(f2=a)), ('ref NULL', dict(ref=None)), ('ref NaN', dict(ref=np.array([0.0, nan]))),
            ('np -1', dict(np_=-1)), ('np 4097', dict(np_=4097)), ('P NULL', dict(P=None)), ('P inf', dict(P=np.array([0.3, 0.1, inf, 0.3]))),
            ('M 0', dict(M=0)), ('Xc NULL', dict(X=False)), ('k 4097', dict(k=4097)), ('top_idx NULL', dict(ti=None)),
            ('f2 not fitted', dict(f2=unfit)), ('f2 d 3', dict(f2=c)),
            ('f1 == f2 + ref NaN', dict(f2=a, ref=np.array([nan, 0.0]))), ('ref NaN + np -1', dict(ref=np.array([nan, 0.0]), np_=-1)),
            ('P NULL + M 0', dict(P=None, M=0)), ('M 0 + k 4097', dict(M=0, k=4097)), ('k 4097 + f2 not fitted', dict(k=4097, f2=unfit)),
            ('f2 not fitted + Xc NULL', dict(f2=unfit, X=False)), ('f1 not fitted, f2 d 3', dict(f1=unfit, f2=c))]
    for label, kw in ebad:
        g_ = dict(egood, **kw)
        f2 = g_['f2']
        out['ehvi host: %s' % label] = _err(lib, g_['f1'], lib.gpx_ehvi_sweep(g_['f1'], f2, _p(g_['P']), g_['np_'], _p(g_['ref']), _p(Xc) if g_['X'] else None,
                                                                               g_['M'], g_['k'], _p(g_['tv']), _p(g_['ti']), None))
        out['ehvi dev: %s' % label] = _err(lib, g_['f1'], lib.gpx_ehvi_sweep_dev(g_['f1'], f2, _p(g_['P']), g_['np_'], _p(g_['ref']), dXc if g_['X'] else None,
                                                                                  g_['M'], g_['k'], _p(g_['tv']), _p(g_['ti']), None, None))
        if not any(key in kw for key in ('f1', 'f2')):      # the fold alone: the lead, the moments (here: any device pointer, never read) and the front
            out['ehvi fold: %s' % label] = _err(lib, a, lib.gpx_ehvi_fold_dev(a, dXc if g_['X'] else None, g_['M'], _p(g_['P']), g_['np_'], _p(g_['ref']),
                                                                              g_['k'], _p(g_['tv']), _p(g_['ti']), None))
    out['ehvi host: f1 NULL'] = [lib.gpx_ehvi_sweep(None, b, _p(front), 2, _p(ref), _p(Xc), M, 5, _p(tv), _p(ti), None), None]
    out['ehvi fold: lead NULL'] = [lib.gpx_ehvi_fold_dev(None, dXc, M, _p(front), 2, _p(ref), 5, _p(tv), _p(ti), None), None]

    sv, si, ss = np.zeros(64), np.zeros(64, dtype=np.int64), np.zeros(2 * 64)
    bgood = dict(mem=[a, b], acq=0, prm=prm, np_=1, nb=2, sv=sv, si=si)
    bbad = [('MES', dict(acq=16)), ('KG', dict(acq=32)), ('MEAN', dict(acq=3)), ('acq 4', dict(acq=4)), ('params NULL', dict(prm=None, np_=0)),
            ('nb 0', dict(nb=0)), ('nb 65', dict(nb=65)), ('sel_val NULL', dict(sv=None)), ('sel_idx NULL', dict(si=None)),
            ('MES + nb 0', dict(acq=16, nb=0)), ('MEAN + params NULL', dict(acq=3, prm=None, np_=0)), ('MEAN + nb 65', dict(acq=3, nb=65)),
            ('nb 65 + sel_val NULL', dict(nb=65, sv=None))]

    def batch(hh, g_):
        return lib.gpx_sweep_batch(hh, g_['acq'], _p(g_['prm']), g_['np_'], g_['nb'], _p(g_['sv']), _p(g_['si']), None, None)

    def ens_batch(g_, n=None):
        return lib.gpx_ensemble_sweep_batch(arr(g_['mem']) if g_['mem'] is not None else None, len(g_['mem'] or ()) if n is None else n, g_['acq'],
                                            _p(g_['prm']), g_['np_'], g_['nb'], _p(g_['sv']), _p(g_['si']), _p(ss))

    for label, kw in bbad:
        out['sweep_batch: %s' % label] = _err(lib, a, batch(a, dict(bgood, **kw)))
        out['ensemble_sweep_batch: %s' % label] = _err(lib, a, ens_batch(dict(bgood, **kw)))
    out['sweep_batch: no cache'] = _err(lib, b, batch(b, bgood))
    out['sweep_batch: no cache + sel_val NULL'] = _err(lib, b, batch(b, dict(bgood, sv=None)))
    out['sweep_batch: not fitted'] = _err(lib, unfit, batch(unfit, bgood))
    out['sweep_batch: handle NULL'] = [batch(None, bgood), None]
    # gpx_sweep_batch_fantasy on `a` (M = 64 cached candidates): S = 4 fantasies, nb = 3 picks, eps wide enough for every probe
    feps = np.random.RandomState(11).randn(65, 32)
    feps_nan = feps.copy()
    feps_nan[1, 1] = nan
    fgood = dict(bgood, h=a, nb=3, eps=feps, S=4, ld=32, inc=1, pend=None, npend=0)
    fbad = [('not fitted', dict(h=unfit)), ('no cache', dict(h=b)), ('nb 0', dict(nb=0)), ('nb 65', dict(nb=65)), ('sel_val NULL', dict(sv=None)),
            ('UCB', dict(acq=2)), ('MES', dict(acq=16)), ('S 0', dict(S=0)), ('S 65', dict(S=65)), ('incumbent 2', dict(inc=2)),
            ('eps NULL', dict(eps=None)), ('ld_eps 1 < nb - 1', dict(ld=1)), ('npend = nb', dict(pend=[0, 1, 2], npend=3)),
            ('pend_idx NULL, npend 1', dict(npend=1)), ('pending row twice', dict(pend=[5, 5], npend=2)),
            ('pending row 64 = M', dict(pend=[64], npend=1)), ('eps NaN', dict(eps=feps_nan)),
            ('no cache + sel_val NULL', dict(h=b, sv=None)), ('no cache + UCB', dict(h=b, acq=2)), ('S 65 + eps NULL', dict(S=65, eps=None))]

    def fantasy(g_):
        pend = None if g_['pend'] is None else np.array(g_['pend'], dtype=np.int64)
        return lib.gpx_sweep_batch_fantasy(g_['h'], g_['acq'], _p(g_['prm']), g_['np_'], g_['nb'], _p(g_['eps']), g_['S'], g_['ld'], g_['inc'],
                                           _p(pend), g_['npend'], _p(g_['sv']), _p(g_['si']), None, None)

    for label, kw in fbad:
        g_ = dict(fgood, **kw)
        out['sweep_batch_fantasy: %s' % label] = _err(lib, g_['h'], fantasy(g_))
    out['sweep_batch_fantasy: handle NULL'] = [fantasy(dict(fgood, h=None)), None]
    out['ensemble_sweep_batch: no cache'] = _err(lib, a, ens_batch(bgood))
    out['ensemble_sweep_batch: no cache on the lead'] = _err(lib, b, ens_batch(dict(bgood, mem=[b, a])))
    out['ensemble_sweep_batch: twice'] = _err(lib, a, ens_batch(dict(bgood, mem=[a, a])))
    out['ensemble_sweep_batch: twice + no cache'] = _err(lib, b, ens_batch(dict(bgood, mem=[b, b])))
    out['ensemble_sweep_batch: n_members 65'] = _err(lib, a, ens_batch(dict(bgood, mem=[a] * 65)))
    out['ensemble_sweep_batch: n_members 65 + MES'] = _err(lib, a, ens_batch(dict(bgood, mem=[a] * 65, acq=16)))
    out['ensemble_sweep_batch: n_members 0'] = _err(lib, a, ens_batch(bgood, n=0))
    out['ensemble_sweep_batch: member NULL'] = _err(lib, a, ens_batch(dict(bgood, mem=[a, None])))
    out['ensemble_sweep_batch: members NULL'] = [ens_batch(dict(bgood, mem=None), n=2), None]
    out['ensemble_sweep_batch: member not fitted'] = _err(lib, a, ens_batch(dict(bgood, mem=[a, unfit])))
    out['ensemble_sweep_batch: member d 3'] = _err(lib, a, ens_batch(dict(bgood, mem=[a, c])))
    out['ensemble_sweep_batch: member not fitted + twice'] = _err(lib, a, ens_batch(dict(bgood, mem=[a, unfit, unfit])))
    out['ensemble_sweep_batch: sel_val NULL + member d 3'] = _err(lib, a, ens_batch(dict(bgood, mem=[a, c], sv=None)))
    assert lib.gpx_set_option(b, b'sweep_cache', 1) == 0          # b: a live cache of another size
    assert lib.gpx_sweep(b, 0, _p(prm), 1, _p(Xc), M // 2, 5, _p(tv), _p(ti), None, None, None) == 0
    out['sweep_batch: nb 33 > M 32'] = _err(lib, b, batch(b, dict(bgood, nb=33)))
    out['sweep_batch_fantasy: nb 33 > M 32'] = _err(lib, b, fantasy(dict(fgood, h=b, nb=33)))
    out['ensemble_sweep_batch: caches differ in size'] = _err(lib, a, ens_batch(bgood))
    out['ensemble_sweep_batch: caches differ in size + nb 64'] = _err(lib, a, ens_batch(dict(bgood, nb=64)))

    nv = 10
    vv = rng.randn(2 * nv)
    pgood = dict(h=a, v=vv, nv=nv, S=2, n=n, d=d, X=True, M=M, k=5)
    pbad = [('not fitted', dict(h=unfit)), ('v NULL', dict(v=None)), ('d 3', dict(d=3)), ('nv 0', dict(nv=0)), ('nv N + 1', dict(nv=11)),
            ('S 0', dict(S=0)), ('n 4097', dict(n=4097)), ('n 0', dict(n=0)), ('k 4097', dict(k=4097)), ('k -1', dict(k=-1)), ('Xc NULL', dict(X=False)),
            ('M 0', dict(M=0)), ('not fitted + v NULL', dict(h=unfit, v=None)), ('v NULL + d 3', dict(v=None, d=3)), ('d 3 + nv 0', dict(d=3, nv=0)),
            ('nv 0 + S 0', dict(nv=0, S=0)), ('S 0 + n 4097', dict(S=0, n=4097)), ('n 4097 + Xc NULL', dict(n=4097, X=False)),
            ('Xc NULL + k 4097', dict(X=False, k=4097)), ('M 0 + k 4097', dict(M=0, k=4097))]
    tvp, tip = np.zeros(2 * 8), np.zeros(2 * 8, dtype=np.int64)
    for form in ('host', 'dev'):
        fn = lib.gpx_path_sweep if form == 'host' else lib.gpx_path_sweep_dev
        for label, kw in pbad:
            g_ = dict(pgood, **kw)
            Xp = None if not g_['X'] else (_p(Xc) if form == 'host' else dXc)
            rc = fn(g_['h'], _p(W), _p(bb), _p(z), _p(g_['v']), g_['nv'], g_['S'], g_['n'], g_['d'], 0.0, Xp, g_['M'], g_['k'], _p(tvp), _p(tip), None)
            out['path_sweep %s: %s' % (form, label)] = _err(lib, g_['h'], rc)
        out['path_sweep %s: W NULL' % form] = _err(lib, a, fn(a, None, _p(bb), _p(z), _p(vv), nv, 2, n, d, 0.0, _p(Xc) if form == 'host' else dXc, M, 5,
                                                           _p(tvp), _p(tip), None))

    lib.gpx_grid_destroy(grid)
    for hh in (unfit, a, b, c):
        lib.gpx_destroy(hh)
    return out


def encode(results):
    """{lib: {case: [rc, message or None, *extras]}} -> the fixture, every message stored once (index, -1 for None)."""
    flat = [x for r in results.values() for v in r.values() for x in (v if isinstance(v[0], list) else [v])]
    msgs = sorted({x[1] for x in flat if x[1] is not None})
    idx = {m: i for i, m in enumerate(msgs)}

    def enc(x):
        return [enc(y) for y in x] if isinstance(x[0], list) else [x[0], -1 if x[1] is None else idx[x[1]]] + x[2:]
    return {'values': VALUES, 'messages': msgs, 'libs': {lib: {k: enc(v) for k, v in r.items()} for lib, r in results.items()}}


def decode(fixture):
    """The fixture -> {lib: {case: [rc, message or None, *extras]}}, as probe() returns it."""
    msgs = fixture['messages']

    def dec(x):
        return [dec(y) for y in x] if isinstance(x[0], list) else [x[0], None if x[1] < 0 else msgs[x[1]]] + x[2:]
    return {lib: {k: dec(v) for k, v in r.items()} for lib, r in fixture['libs'].items()}


def rows(fixture):
    return sum(len(v) if isinstance(v[0], list) else 1 for r in fixture['libs'].values() for v in r.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ship', default=os.path.join(CSRC, 'libgpx.so'))
    ap.add_argument('--diag', default=os.path.join(CSRC, 'libgpx_diag.so'))
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    ship, diag = probe(args.ship), probe(args.diag)
    fixture = encode({'ship': ship, 'diag': diag})
    assert decode(json.loads(json.dumps(fixture))) == {'ship': ship, 'diag': diag}
    with open(args.out, 'w') as f:
        json.dump(fixture, f, separators=(',', ':'))
        f.write('\n')
    print('wrote %s: %d rows, %d messages, %d bytes' % (args.out, rows(fixture), len(fixture['messages']), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
