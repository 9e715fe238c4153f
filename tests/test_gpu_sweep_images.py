"""The two-image k-loop of the default sweep schedule (option "sweep_images", pybo_amd/csrc/gemm_core.h: gemm_tile_128_l2, kernels_sweep.hip:
k_sweep_trmm_l2) changes when a k-step's operands arrive in LDS and nothing else: per accumulator block the MFMAs, their operands and
their order along k are those of the single-image loop at every tile width.  So every output of a sweep must be array_equal between
sweep_images = 1 and 2 at sweep_cols = 128, 64 and 32 -- all six combinations -- at the smallest shapes at which the loop can go wrong
(tile_order 19 forced, chunk = 4096, as tests/test_gpu_sweep_narrow.py):

  N = 100   1 block row: a single tile whose 4 k-steps are the triangular block's quarters (no full step but the first: nd = 1)
  N = 300   3 block rows: a pair of unequal length and the odd middle tile alone
  N = 1300  11 block rows: the down-rule off
  N = 4100  33 block rows, the last one padded; tiles on both sides of 2 mt < nP - 1: descending steps with the skip sequence 3, 2, 1, 0, ..
  M = 31, 33, 129, 1000, 4096 + 17 (test_gpu_sweep_narrow.py: why); NaN coordinates and duplicated candidates; a refused value.

Row prefix (N = 4100, prune = 1, prune_rows = 16, M = 20000, the length scales halved as in tests/test_gpu_prune_rows.py so that
the first level prunes instead of falling back): the second bound's vectors (gpx_prune_rows: qR, ub2, idx2), the survivor
counts and the final top-k are the same at the six combinations, on a first-level list of more than 256 candidates, i.e. several
panels and, 32 wide, more than one tile per XCD (first run on the device: nsurv = 4855, nsurv2 = 0).

All assertions are array_equal."""
import numpy as np
import pytest

from pybo_amd import _lib
from test_gpu_prune import _dev
from test_gpu_prune_bound import _engine, _problem

pytestmark = pytest.mark.gpu

K = 10
SIZES = (31, 33, 129, 1000, 4096 + 17)
SHAPES = [(cols, images) for cols in (128, 64, 32) for images in (1, 2)]


def _outputs(e, target, Z, cols, images):
    e.set_option('sweep_cols', cols)
    e.set_option('sweep_images', images)
    r = e.sweep('ei', target, Z, k=K, want_all=True, want_moments=True)
    top = e.sweep('ei', target, Z, k=K, want_all=False)              # the top-k alone
    e.set_option('sweep_cols', -1)
    e.set_option('sweep_images', -1)
    r['only_val'], r['only_idx'] = top['top_val'], top['top_idx']
    return r


def _assert_same(a, b, label):
    for name in ('acq', 'mu', 's2', 'top_val', 'top_idx', 'only_val', 'only_idx'):
        assert np.array_equal(a[name], b[name], equal_nan=not name.endswith('idx')), (label, name)
    assert np.array_equal(a['top_idx'], a['only_idx']) and np.array_equal(a['top_val'], a['only_val'], equal_nan=True), label


def _compare(e, target, Z, label):
    first = _outputs(e, target, Z, *SHAPES[0])
    for cols, images in SHAPES[1:]:
        _assert_same(first, _outputs(e, target, Z, cols, images), '%s sweep_cols=%d sweep_images=%d' % (label, cols, images))
    return first


@pytest.fixture(scope='module', params=[100, 300, 1300, 4100], ids=['nP1', 'nP3', 'nP11', 'nP33'])
def fitted(request):
    N = request.param
    w = _problem(N, 4, max(SIZES), 'se', seed=N)
    e = _engine(w, tile_order=19, chunk=4096)
    yield N, w, e, float(np.max(w['y']))
    e.close()


@pytest.mark.parametrize('M', SIZES)
def test_per_candidate_outputs_are_the_same_bits_at_every_width_and_image_count(fitted, M):
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


def test_an_image_count_that_does_not_exist_is_refused(fitted):
    e = fitted[2]
    for bad in (0, 3, 4, -2, 128):
        with pytest.raises(_lib.GpxError) as err:
            e.set_option('sweep_images', bad)
        assert err.value.code == _lib.GPX_EARG, bad
    e.set_option('sweep_images', -1)


def test_row_prefix_launch_writes_the_same_bits_in_every_shape():
    N, M, rows = 4100, 20000, 16
    w = _problem(N, 4, M, 'se', seed=N)
    w['ell'] = w['ell'] * 0.5                 # (unscaled, 10594 candidates survive the first level: more than cap = M / 4, no second level)
    e = _engine(w, tile_order=19, chunk=4096, prune=1, prune_rows=rows)
    target = e.mean_at_obs()[1]
    dZ = _dev(w['Xc'])
    first = None
    for cols, images in SHAPES:
        e.set_option('sweep_cols', cols)
        e.set_option('sweep_images', images)
        val, idx = e.sweep_dev('ei', target, dZ.data_ptr(), M, K)[:2]
        r = e.prune_report()
        label = 'sweep_cols=%d sweep_images=%d' % (cols, images)
        assert r['path'] == 'pruned' and r['nR'] == rows and r['nsurv'] > 256, (label, r['path'], r['nR'], r['nsurv'])
        got = dict(val=val, idx=idx, qR=r['qR'], ub2=r['ub2'], idx2=r['idx2'], list=r['idx'], counts=np.array([r['nsurv'], r['nsurv2'], r['G']]))
        if first is None:
            first = got
            print('row prefix: nsurv %d nsurv2 %d G %d' % (r['nsurv'], r['nsurv2'], r['G']))
            assert np.all(np.isfinite(got['qR'])) and np.all(got['qR'] > 0.0)      # real sums
            continue
        for name in got:
            assert np.array_equal(first[name], got[name], equal_nan=name in ('val', 'ub2', 'qR')), (label, name)
    e.close()
