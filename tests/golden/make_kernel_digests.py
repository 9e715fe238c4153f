"""Bit-exact digests of what the triangular inverse and the sweep kernels produce, recorded from the commit BEFORE the sweep
kernels got one frame and the inverse's eight product kernels became one template: a refactor of kernels must leave every
bit where it was, and the tolerance tests would not notice an equally accurate but different result.

    inverse   get_matrix('L'), get_matrix('T'), get_vectors() for N = 300 (3 block rows), 1000, 2500 (20, not a power of two),
              5000 (40: a short trailing group), 8192 (64: levels below 32 on 64-tiles, level 32 on 128-tiles), each with
              trtri_left 0 and 1 and, from 8 block rows on, with the leading part riding behind the factorisation
              (trtri_ahead 1; the number of times it did is part of the record); refine_inverse once at N = 2500; N = 1000 with
              chol_tg_db 0 and 1 (the default, -1, means the two-image workers at every size here: nothing else runs their
              one-image k-loop)
    sweep     acq, mu, s2 of M = 4096 uniform candidates and the top-10 pairs for N = 1000 (nothing walks downwards) and
              N = 4224 (33 block rows: the downward rule is live), one k-loop schedule per kernel template and -1 (by size)
    rff       the sweep of one set of four posterior draws (n = 100 features: k_rff_mfma5)

Output: tests/golden/kernel_digests.json, per case the SHA-256 of the raw bytes of each output.  Needs a GPU.  Record it from
the PARENT commit's diagnostics library, never from the one under test; tests/test_gpu_kernel_digests.py replays the cases:
    GPX_LIB_PATH=<parent>/pybo_amd/csrc/libgpx_diag.so python tests/golden/make_kernel_digests.py --commit <hash> [--out file.json]
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

OUT = os.path.join(HERE, 'kernel_digests.json')
INVERSE_N = [300, 1000, 2500, 5000, 8192]
AHEAD_MIN_N = 897                      # 8 block rows of 128: the default trtri_ahead_min
SWEEP_N = [1000, 4224]
TILE_ORDERS = [7, 15, 19, 31, 11, 23, 27, -1]      # _w, _l without the skip, _l, _l k-step 16, k_sweep_trmm<2|5|6>, by size
M, D, TOPK = 4096, 5, 10


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _problem(N, seed):
    rng = np.random.RandomState(seed)
    X = rng.rand(N, D)
    y = np.sin(3.0 * X.sum(1)) + 0.5 * np.cos(5.0 * X[:, 0]) + 1e-2 * rng.randn(N)
    return X, y, 0.3 + 0.2 * rng.rand(D)


def _engine(**opts):
    from pybo_amd._lib import Engine
    e = Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _inverse(N, **opts):
    X, y, ell = _problem(N, seed=N)
    e = _engine(eager_inverse=1, **opts)
    e.fit(X, y, 'se', ell, 1.3, 1e-3, 0.2)
    tm = e.timers(reset=True)
    a, alpha = e.get_vectors()
    out = dict(L=_sha(e.get_matrix('L')), T=_sha(e.get_matrix('T')), a=_sha(a), alpha=_sha(alpha),
               ahead=int(tm['trtri_ahead']), chol_fallbacks=int(tm['chol_fallbacks']))
    e.close()
    return out


def _sweep(N):
    X, y, ell = _problem(N, seed=N)
    Xc = np.random.RandomState(N + 1).rand(M, D)
    e = _engine()
    e.fit(X, y, 'se', ell, 1.3, 1e-3, 0.2)
    out = {}
    for order in TILE_ORDERS:
        e.set_option('tile_order', order)
        r = e.sweep('ei', float(y.max()), Xc, k=TOPK, want_all=True, want_moments=True)
        out['tile_order %d' % order] = {k: _sha(r[k]) for k in ('acq', 'mu', 's2', 'top_val', 'top_idx')}
    e.close()
    return out


def _rff():
    rng = np.random.RandomState(11)
    S, n = 4, 100
    W, b, theta = rng.randn(S, n, D) / 0.4, 2 * np.pi * rng.rand(S, n), rng.randn(S, n)
    e = _engine()
    r = e.rff_sweep(W, b, theta, 0.1, rng.rand(M, D), k=TOPK)
    e.close()
    return {k: _sha(r[k]) for k in ('vals', 'top_val', 'top_idx')}


def cases():
    """[(name, thunk)]: every thunk returns {output: digest or count} (the sweep's: one such dict per schedule)."""
    out = []
    for N in INVERSE_N:
        out.append(('inverse N=%d' % N, lambda N=N: _inverse(N, trtri_ahead=0)))
        out.append(('inverse N=%d left' % N, lambda N=N: _inverse(N, trtri_ahead=0, trtri_left=1)))
        if N >= AHEAD_MIN_N:
            out.append(('inverse N=%d ahead' % N, lambda N=N: _inverse(N, trtri_ahead=1)))
    out.append(('inverse N=2500 refined', lambda: _inverse(2500, refine_inverse=1)))
    for db in (0, 1):                      # the factorisation's workers forced onto the one-image / the two-image k-loop
        out.append(('inverse N=1000 db%d' % db, lambda db=db: _inverse(1000, trtri_ahead=0, chol_tg_db=db)))
    for N in SWEEP_N:
        out.append(('sweep N=%d' % N, lambda N=N: _sweep(N)))
    out.append(('rff sweep', _rff))
    return out


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
        flat = lambda r: {(k, kk): vv for k, v in r.items() for kk, vv in (v.items() if isinstance(v, dict) else [(None, v)])}
        unstable = sorted(str(k) for k in flat(first) if flat(first)[k] != flat(second)[k])
        if unstable:
            print('NOT reproducible in %s: %s' % (name, unstable), file=sys.stderr)
            for k in list(first):
                if isinstance(first[k], dict):
                    first[k] = {kk: vv for kk, vv in first[k].items() if second[k][kk] == vv}
                elif first[k] != second[k]:
                    del first[k]
        if name.endswith('ahead'):
            assert first['ahead'] == 1, (name, first)
        doc['cases'][name] = first
        print(name, 'ok', flush=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s (%d cases)' % (args.out, len(doc['cases'])))


if __name__ == '__main__':
    main()
