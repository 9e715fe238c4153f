"""Narrow candidate tiles of the default sweep schedule (option "sweep_cols", pybo_amd/csrc/kernels_sweep.hip: sweep_tiles) change how
many candidates a workgroup computes and nothing else: per wave the rows, the k-step order, the diagonal block's skip, the up/down rule
and the sequence of MFMAs along k of every accumulator block are the wide tile's, and no column of a tile enters another column's sums.
So every output of a sweep must be array_equal with sweep_cols = 128, 64 and 32, at the smallest shapes at which a width can go wrong:

  N = 4100 (33 block rows, the last one padded; tiles on both sides of the down-rule 2 mt < nP - 1) and N = 1300 (11 block rows, rule
  off), tile_order 19 forced;
  M = 31 and 33 (less and more than one narrowest tile), 129 (a second panel of one column), 1000 (a ragged last tile at both narrow
  widths: 1000 = 15 x 64 + 40 = 31 x 32 + 8), 4096 + 17 (a second chunk of one ragged tile at chunk = 4096; 4096 ends a panel);
  NaN coordinates and duplicated candidates;  a refused width.

All assertions are array_equal."""
import numpy as np
import pytest

from pybo_amd import _lib
from test_gpu_prune_bound import _engine, _problem

pytestmark = pytest.mark.gpu

K = 10
SIZES = (31, 33, 129, 1000, 4096 + 17)


def _outputs(e, target, Z, cols):
    e.set_option('sweep_cols', cols)
    r = e.sweep('ei', target, Z, k=K, want_all=True, want_moments=True)
    top = e.sweep('ei', target, Z, k=K, want_all=False)              # the top-k alone
    e.set_option('sweep_cols', -1)
    r['only_val'], r['only_idx'] = top['top_val'], top['top_idx']
    return r


def _assert_same(a, b, label):
    for name in ('acq', 'mu', 's2', 'top_val', 'top_idx', 'only_val', 'only_idx'):
        assert np.array_equal(a[name], b[name], equal_nan=not name.endswith('idx')), (label, name)
    assert np.array_equal(a['top_idx'], a['only_idx']) and np.array_equal(a['top_val'], a['only_val'], equal_nan=True), label


def _compare(e, target, Z, label):
    wide = _outputs(e, target, Z, 128)
    for cols in (64, 32):
        _assert_same(wide, _outputs(e, target, Z, cols), '%s sweep_cols=%d' % (label, cols))
    return wide


@pytest.fixture(scope='module', params=[4100, 1300], ids=['nP33', 'nP11'])
def fitted(request):
    N = request.param
    w = _problem(N, 4, max(SIZES), 'se', seed=N)
    e = _engine(w, tile_order=19, chunk=4096)
    yield N, w, e, float(np.max(w['y']))
    e.close()


@pytest.mark.parametrize('M', SIZES)
def test_per_candidate_outputs_are_the_same_bits_at_every_width(fitted, M):
    N, w, e, target = fitted
    r = _compare(e, target, w['Xc'][:M], 'N=%d M=%d' % (N, M))
    assert np.all(np.isfinite(r['mu'])) and np.all(r['s2'] > 0.0)              # real sums were compared, not NaN with NaN


def test_nan_coordinates_and_duplicates(fitted):
    N, w, e, target = fitted
    M = 1000
    Z = w['Xc'][:M].copy()
    best = np.argsort(-e.sweep('ei', target, Z, k=0, want_all=True)['acq'], kind='stable')[:2]
    Zn = Z.copy()
    Zn[[int(best[0]), 5, 63, 64, 999], 1] = np.nan
    Zn[[31, 32, 500], 2] = -np.nan
    nan_rows = sorted(set([int(best[0]), 5, 31, 32, 63, 64, 500, 999]))
    r = _compare(e, target, Zn, 'N=%d NaN' % N)
    assert np.array_equal(np.flatnonzero(np.isnan(r['mu'])), nan_rows) and np.array_equal(np.flatnonzero(np.isnan(r['acq'])), nan_rows)
    Zd = Z.copy()
    Zd[[0, 31, 32, 63, 64, 999]] = Z[best[0]]
    Zd[[1, 998]] = Z[best[1]]
    same = sorted(set([0, 31, 32, 63, 64, 999, int(best[0])]))
    r = _compare(e, target, Zd, 'N=%d duplicates' % N)
    assert sorted(int(i) for i in r['top_idx'][:len(same)]) == same
    assert len(set(r['acq'][same])) == 1                      # one candidate, one value, whatever column it sits in


def test_a_width_that_does_not_exist_is_refused(fitted):
    e = fitted[2]
    for bad in (0, 16, 48, 96, 127, 256, -2):
        with pytest.raises(_lib.GpxError) as err:
            e.set_option('sweep_cols', bad)
        assert err.value.code == _lib.GPX_EARG, bad
    e.set_option('sweep_cols', -1)
