"""Bit-exact digests of the per-candidate arithmetic behind every acquisition, recorded from the commit BEFORE that arithmetic
(sums and moments, the variance floor, the ensemble's fold and finish, the total order and its arg-max, a pick's record) moved
into pybo_amd/csrc/acq_core.h: the move must leave every bit where it was.  What kernel_digests.json and select_digests.json
do not pin:

    single, cold    pi, ucb, mean with moments; mes with S = 1, 3, 64; kg with m = 1 and m = 6 support points on se and matern5
    seeded caches   a sweep with sweep_cache = 1 by each of ei, mes, kg, two appends, then sweep_update for ei and mes (the cache
                    form of the moments: no row blocks left to add)
    batch           sweep_batch, nb = 4, for ei, pi, ucb with s2_all
    fantasy         sweep_batch_fantasy, nb = 4, for ei and pi over S = 1 (one ragged chunk), 5, 16 (one full chunk) and 17 (two chunks,
                    one live lane in the second) fantasies, eps = RandomState(23).randn(S, 3), each with incumbent 0 and 1 and with
                    s2_all; one case with two pending rows and one with nb = 1 (no conditioning, eps unread)
    ensemble        three members (N = 300, 300, 100; their own ell, rho, bias): ensemble_sweep for ei, pi, mean, ucb (mean and ucb
                    with the mixture moments), mes with S = 2 per member; ensemble_batch, nb = 4, for ei, pi and ucb
    predict         with gradients at one point (the one-pass form) and at five (the two-pass form), and both forms forced

d = 5; N = 300 (three row blocks) and N = 100 (one); M = 4099 uniform candidates under chunk = 1024 (five chunks, the last with
three valid columns).  Every sweep runs on a grid whose last three rows repeat its best row, so the four best values are equal
and the order's tie rule decides: the recorder and the replay both assert top_idx[:4] = [best, M - 3, M - 2, M - 1].

Output: tests/golden/acq_digests.json, per case the SHA-256 of the raw bytes of each output.  Needs a GPU.  Record it from the
PARENT commit's diagnostics library, never from the one under test; tests/test_gpu_acq_digests.py replays the cases:
    GPX_LIB_PATH=<parent>/pybo_amd/csrc/libgpx_diag.so python tests/golden/make_acq_digests.py --commit <hash> [--out file.json]
Every case runs twice and the recorder fails if the two runs differ anywhere: no output is left out.
Cases added after the first recording (the fantasy rows and the ensemble batch for pi, from the commit before the batch kernels
got one frame) go in with --add: every case runs, the rows the file already holds must come out as recorded and stay, and the
new ones are listed under "added" by the commit that produced them.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, 'acq_digests.json')
M, D, TOPK, CHUNK, NB = 4099, 5, 10, 1024, 4
SN2 = 1e-3
SWEEP_KEYS = ('acq', 'mu', 's2', 'top_val', 'top_idx')
# the ensemble's members: (N, scale of ell, rho, bias)
MEMBERS = [(300, 1.0, 1.3, 0.2), (300, 0.7, 0.9, -0.1), (100, 1.4, 1.7, 0.05)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digest(r, keys):
    return {k: _sha(r[k]) for k in keys if r.get(k) is not None}


def _problem(N):
    rng = np.random.RandomState(1000 + N)
    X = rng.rand(N + 2, D)                      # (the last two rows: the appends)
    y = np.sin(3.0 * X.sum(1)) + 0.5 * np.cos(5.0 * X[:, 0]) + 1e-2 * rng.randn(N + 2)
    return X, y, 0.3 + 0.2 * rng.rand(D)


def _grid():
    return np.random.RandomState(77).rand(M, D)


def _engine(N, kernel='se', scale=1.0, rho=1.3, bias=0.2):
    from pybo_amd._lib import Engine
    X, y, ell = _problem(N)
    e = Engine(0)
    e.set_option('chunk', CHUNK)
    e.fit(X[:N], y[:N], kernel, scale * ell, rho, SN2, bias)
    return e


def _target(N):
    return float(_problem(N)[1][:N].max())


def _maxima(N, S, shift=0.0):
    return _target(N) + shift + 0.05 * np.arange(1, S + 1)


def _support(m):
    return np.random.RandomState(5).rand(m, D)


def _tied(sweep):
    """sweep(Z) -> a result with top_idx.  Runs it on the plain grid, repeats the best row in the last three rows and runs it again:
    (the tied grid, that second result), the tie rule asserted."""
    Z = _grid()
    best = int(sweep(Z)['top_idx'][0])
    assert 0 <= best < M - 3, best
    Z[M - 3:] = Z[best]
    r = sweep(Z)
    want = [best, M - 3, M - 2, M - 1]
    assert list(r['top_idx'][:4]) == want, ('the tie rule: top_idx[:4] is %s, not %s' % (list(r['top_idx'][:4]), want))
    assert len({float(v).hex() for v in r['top_val'][:4]}) == 1, r['top_val'][:4]
    return Z, r


def _cold(N, acq, param, kernel='se', moments=True):
    e = _engine(N, kernel)
    _, r = _tied(lambda Z: e.sweep(acq, param, Z, k=TOPK, want_all=True, want_moments=moments))
    e.close()
    return _digest(r, SWEEP_KEYS)


def _seeded(N, acq, param):
    e = _engine(N)
    e.set_option('sweep_cache', 1)
    _, r = _tied(lambda Z: e.sweep(acq, param, Z, k=TOPK, want_all=True, want_moments=True))
    e.set_option('sweep_cache', 0)
    assert e.sweep_cache_size() == M
    X, y, _ = _problem(N)
    for i in (N, N + 1):
        assert e.append(X[i], y[i])
    out = {'seed ' + k: v for k, v in _digest(r, SWEEP_KEYS).items()}
    for name, p in (('ei', _target(N)), ('mes', _maxima(N, 3))):
        u = e.sweep_update(name, p, k=TOPK, want_all=True, want_moments=True)
        out.update({'%s %s' % (name, k): v for k, v in _digest(u, SWEEP_KEYS).items()})
    e.close()
    return out


def _batch(N, kind, param):
    e = _engine(N)
    e.set_option('sweep_cache', 1)
    _tied(lambda Z: e.sweep('ei', _target(N), Z, k=TOPK, want_all=False))
    e.set_option('sweep_cache', 0)
    r = e.sweep_batch(kind, param, NB, want_s2_all=True)
    e.close()
    return _digest(r, BATCH_KEYS)


BATCH_KEYS = ('sel_val', 'sel_idx', 'sel_s2', 's2_all')
PENDING = (7, 2048)


def _fantasy(N, kind, S, incumbents, nb=NB, pending=None):
    e = _engine(N)
    e.set_option('sweep_cache', 1)
    _tied(lambda Z: e.sweep('ei', _target(N), Z, k=TOPK, want_all=False))
    e.set_option('sweep_cache', 0)
    eps = np.random.RandomState(23).randn(S, 3)
    out = {}
    for inc in incumbents:
        r = e.sweep_batch_fantasy(kind, _target(N), nb, eps, incumbent=inc, pending=pending, want_s2_all=True)
        out.update({'incumbent %d %s' % (inc, k): v for k, v in _digest(r, BATCH_KEYS).items()})
    e.close()
    return out


def _members():
    return [_engine(N, 'se', scale, rho, bias) for N, scale, rho, bias in MEMBERS]


def _ens_sweep(acq, param, moments):
    from pybo_amd._lib import Engine
    engines = _members()
    _, r = _tied(lambda Z: Engine.ensemble_sweep(engines, acq, param, Z, k=TOPK, want_all=True, want_moments=moments))
    for e in engines:
        e.close()
    return _digest(r, SWEEP_KEYS)


def _ens_batch(kind, param):
    from pybo_amd._lib import Engine
    engines = _members()
    Z, _ = _tied(lambda Z: Engine.ensemble_sweep(engines, 'ei', _target(300), Z, k=TOPK, want_all=True))
    for e in engines:
        e.set_option('sweep_cache', 1)
        e.sweep('ei', _target(300), Z, k=1, want_all=False)
        e.set_option('sweep_cache', 0)
    r = Engine.ensemble_batch(engines, kind, param, NB)
    for e in engines:
        e.close()
    return _digest(r, ('sel_val', 'sel_idx', 'sel_s2'))


def _predict(npts, form):
    e = _engine(300)
    e.set_option('grad_form', form)
    mu, s2, dmu, ds2 = e.predict(_grid()[:npts], grad=True)
    e.close()
    return dict(mu=_sha(mu), s2=_sha(s2), dmu=_sha(dmu), ds2=_sha(ds2))


def cases():
    """[(name, thunk)]: every thunk returns {output: digest}."""
    out = []
    for N in (300, 100):
        t = _target(N)
        for acq, param in (('pi', t), ('ucb', 2.0), ('mean', None)):
            out.append(('cold %s N=%d' % (acq, N), lambda N=N, acq=acq, param=param: _cold(N, acq, param)))
        for S in (1, 3, 64):
            out.append(('cold mes S=%d N=%d' % (S, N), lambda N=N, S=S: _cold(N, 'mes', _maxima(N, S))))
        for m in (1, 6):
            for kernel in ('se', 'matern5'):
                out.append(('cold kg m=%d %s N=%d' % (m, kernel, N), lambda N=N, m=m, kernel=kernel: _cold(N, 'kg', _support(m), kernel)))
        for acq, param in (('ei', t), ('mes', _maxima(N, 3)), ('kg', _support(6))):
            out.append(('cache seeded by %s N=%d' % (acq, N), lambda N=N, acq=acq, param=param: _seeded(N, acq, param)))
        for kind, param in (('ei', t), ('pi', t), ('ucb', 2.0)):
            out.append(('batch %s N=%d' % (kind, N), lambda N=N, kind=kind, param=param: _batch(N, kind, param)))
        for kind in ('ei', 'pi'):
            for S in (1, 5, 16, 17):
                out.append(('fantasy %s S=%d N=%d' % (kind, S, N), lambda N=N, kind=kind, S=S: _fantasy(N, kind, S, (0, 1))))
    out.append(('fantasy ei S=5 N=300 pending', lambda: _fantasy(300, 'ei', 5, (1,), pending=PENDING)))
    out.append(('fantasy ei S=5 N=300 nb=1', lambda: _fantasy(300, 'ei', 5, (1,), nb=1)))
    t = _target(300)
    for acq, param, moments in (('ei', t, False), ('pi', t, False), ('mean', None, True), ('ucb', 2.0, True)):
        out.append(('ensemble %s' % acq, lambda acq=acq, param=param, moments=moments: _ens_sweep(acq, param, moments)))
    ys = np.array([_maxima(N, 2, 0.1 * i) for i, (N, _, _, _) in enumerate(MEMBERS)])
    out.append(('ensemble mes S=2', lambda: _ens_sweep('mes', ys, False)))
    for kind, param in (('ei', t), ('pi', t), ('ucb', 2.0)):
        out.append(('ensemble batch %s' % kind, lambda kind=kind, param=param: _ens_batch(kind, param)))
    for npts, form in ((1, 0), (5, 0), (5, 1), (5, 2)):
        out.append(('predict grad %d points form %d' % (npts, form), lambda npts=npts, form=form: _predict(npts, form)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit the loaded library was built from')
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--add', action='store_true', help='keep the rows of --out (they must replay) and add the cases it lacks')
    args = ap.parse_args()
    from pybo_amd import _lib
    doc = dict(commit=args.commit, library=os.path.basename(_lib.LIB_PATH), cases={})
    old = {}
    if args.add:
        with open(args.out) as f:
            doc = json.load(f)
        old = dict(doc['cases'])
        assert doc['library'] == os.path.basename(_lib.LIB_PATH), doc['library']
    for name, run in cases():
        first, second = run(), run()
        unstable = sorted(k for k in first if first[k] != second.get(k))
        if unstable or sorted(first) != sorted(second):
            sys.exit('NOT reproducible in %s: %s -- a finding about the recording library; nothing was written' % (name, unstable))
        if name in old and first != old[name]:
            sys.exit('%s does not replay the recorded row: nothing was written' % name)
        doc['cases'][name] = first
        print(name, 'ok', sorted(first), flush=True)
    new = sorted(set(doc['cases']) - set(old))
    if args.add and new:
        doc.setdefault('added', {})[args.commit] = new
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s (%d cases)' % (args.out, len(doc['cases'])))


if __name__ == '__main__':
    main()
