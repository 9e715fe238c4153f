"""The short form of tile map 3 (pybo_amd/csrc/sweep_map.h, diagnostic option "short_map") changes which workgroup computes a tile
and nothing else: a tile's bits depend on its rows of U, its cross-Gram panel, its K-extent and the up/down rule.  So every
output of a sweep must be array_equal with short_map = 0 (the long form everywhere) and short_map = 1 (the short form wherever
map 3 is in use), at the smallest shapes at which the map can go wrong:

  N = 4096 (32 block rows: the lower half's tiles walk k downwards) and N = 4224 (33: a lone middle tile), tile_order 19, chunks of
  1, 2, 3, 8 and 16 candidate tiles, M = chunk (one launch) and chunk + 77 (a second launch of one ragged tile);
  N = 640 (5 block rows: fewer pair rows than XCDs) with tile_order 19 forced, and on the three-workgroups-per-CU loop (31);
  super_m 4 and 16;  a pruned selection-only sweep with a row-prefix launch (nR = 8 < nP);  a two-member ensemble on the
  default schedule of N = 2048 (the barrier-free loop).

tests/test_sweep_map_host.py proves the map itself on the host; this file holds the device code to it.  All assertions are
array_equal."""
import numpy as np
import pytest

from test_gpu_prune_bound import _engine, _problem
from test_gpu_prune_rows import _scaled

pytestmark = pytest.mark.gpu

CHUNKS = (128, 256, 384, 1024, 2048)
K = 10


def _outputs(e, target, Z, short):
    e.set_option('short_map', short)
    r = e.sweep('ei', target, Z, k=K, want_all=True, want_moments=True)
    e.set_option('short_map', -1)
    return r


def _assert_same(a, b, label):
    for name in ('acq', 'mu', 's2', 'top_val', 'top_idx'):
        assert np.array_equal(a[name], b[name], equal_nan=(name != 'top_idx')), (label, name)
    assert np.all(np.isfinite(a['mu'])) and np.all(a['s2'] > 0.0), label       # real sums were compared, not NaN with NaN


def _compare(e, w, chunk, M, label, short=1):
    e.set_option('chunk', chunk)
    Z = w['Xc'][:M]
    target = float(np.max(w['y']))
    long_form = _outputs(e, target, Z, 0)
    _assert_same(long_form, _outputs(e, target, Z, short), label)
    return long_form


@pytest.mark.parametrize('N', [4096, 4224], ids=['nP32', 'nP33'])
def test_per_candidate_outputs_are_the_same_bits_on_the_default_schedule(N):
    w = _problem(N, 4, max(CHUNKS) + 77, 'se', seed=N)
    e = _engine(w, tile_order=19)
    for chunk in CHUNKS:
        for M in (chunk, chunk + 77):
            r = _compare(e, w, chunk, M, 'N=%d chunk=%d M=%d' % (N, chunk, M))
            # by size (the default) is one of the two forms: the same bits again
            _assert_same(r, _outputs(e, float(np.max(w['y'])), w['Xc'][:M], -1), 'N=%d chunk=%d M=%d by size' % (N, chunk, M))
    e.close()


@pytest.mark.parametrize('tile_order', [19, 31], ids=['two_per_cu', 'three_per_cu'])
def test_fewer_pair_rows_than_xcds(tile_order):
    N = 640
    w = _problem(N, 4, 384 + 77, 'se', seed=N)
    e = _engine(w, tile_order=tile_order)
    for chunk in (128, 384):
        for M in (chunk, chunk + 77):
            _compare(e, w, chunk, M, 'N=640 tile_order=%d chunk=%d M=%d' % (tile_order, chunk, M))
    e.close()


@pytest.mark.parametrize('super_m', [4, 16])
def test_other_super_tile_shapes(super_m):
    N = 4096
    w = _problem(N, 4, 1024 + 77, 'se', seed=N + super_m)
    e = _engine(w, tile_order=19, super_m=super_m)
    _compare(e, w, 1024, 1024 + 77, 'super_m=%d' % super_m)
    e.close()


def test_pruned_sweep_with_a_row_prefix_launch():
    """prune = 1, prune_rows = 8 at N = 4096: the gate's and the seeds' generation, the prefix launch (nR = 8 of nP = 32 block rows)
    and the survivors' launch all take the short form under short_map = 1; the top-k and every count of the report stay."""
    from test_gpu_prune import _dev
    N, M = 4096, 40961
    w = _scaled(N, M, 0.35, 4096)
    e = _engine(w, tile_order=19, prune=1, prune_rows=8)
    target = e.mean_at_obs()[1]
    dZ = _dev(w['Xc'])
    got = {}
    for short in (0, 1):
        e.set_option('short_map', short)
        tv, ti = e.sweep_dev('ei', target, dZ.data_ptr(), M, K)
        got[short] = (tv, ti, e.prune_report())
    e.set_option('prune', 0)
    plain = e.sweep_dev('ei', target, dZ.data_ptr(), M, K)
    (v0, i0, r0), (v1, i1, r1) = got[0], got[1]
    assert r0['path'] == 'pruned' and r0['nR'] == 8 and 0 < r0['nsurv2'] <= r0['nsurv'], (r0['path'], r0['nR'], r0['nsurv'], r0['nsurv2'])
    assert np.array_equal(v0, v1) and np.array_equal(i0, i1)
    assert np.array_equal(v0, plain[0]) and np.array_equal(i0, plain[1])
    for name in ('path', 'M', 'k', 'G', 'Gg', 'done', 'cap', 'nsurv', 'nR', 'nsurv2', 'tau', 'delta', 'S'):
        assert r0[name] == r1[name], name
    for name in ('idx', 'idx2', 'ub', 'ub2', 'qR'):
        assert np.array_equal(r0[name], r1[name], equal_nan=True), name
    e.close()


def test_two_member_ensemble_on_the_default_schedule():
    from pybo_amd._lib import Engine
    N, M = 2048, 2048 + 77
    w = _problem(N, 4, M, 'se', seed=7)
    engines = [_engine(w, chunk=1024), _engine(dict(w, ell=w['ell'] * 0.7, rho=w['rho'] * 1.5), chunk=1024)]
    target = float(np.max(w['y']))
    out = {}
    for short in (0, 1):
        for e in engines:
            e.set_option('short_map', short)
        # EI: the average of the members' values; UCB: the mixture moments (the only ensemble calls that return mu and s2)
        out[short] = (Engine.ensemble_sweep(engines, 'ei', target, w['Xc'], k=K, want_all=True),
                      Engine.ensemble_sweep(engines, 'ucb', 2.0, w['Xc'], k=K, want_all=True, want_moments=True))
    for name in ('acq', 'top_val', 'top_idx'):
        assert np.array_equal(out[0][0][name], out[1][0][name]), ('ensemble ei', name)
    _assert_same(out[0][1], out[1][1], 'ensemble ucb')
    assert np.all(np.isfinite(out[0][0]['acq']))
    for e in engines:
        e.close()
