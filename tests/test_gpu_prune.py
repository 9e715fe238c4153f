"""Selection-only sweeps (option "prune"): an EI sweep that returns only its top-k skips the
candidates whose bound EI(mu + delta, sqrt(rho)) cannot reach the k-th best exactly evaluated value.  The pruned path
must return BIT FOR BIT what the plain loop returns -- values, indices, order -- and must really leave the work out.
Every comparison here is array_equal; the only figure is the share of the N^2 M product that ran, with the bound the
issue set (3 % on the north-star workload, exactly 1 where the gate declines)."""
import numpy as np
import pytest

from oracle import gp_ref
import bench
from helpers import synth_problem

pytestmark = pytest.mark.gpu

KS = (1, 10, 64, 4096)


class _DevBuf(object):
    """n doubles of device memory through the HIP runtime the library has loaded (no second runtime in the process)."""
    _hip = None

    def __init__(self, n):
        import ctypes as C
        if _DevBuf._hip is None:
            from pybo_amd import _lib
            _lib.load()
            hip = C.CDLL('libamdhip64.so')
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            _DevBuf._hip = hip
        self.n = int(n)
        p = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(p), 8 * max(self.n, 1)) == 0
        self.p = p

    def data_ptr(self):
        return self.p.value

    def at(self, i):
        return self.p.value + 8 * int(i)

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        assert self._hip.hipMemcpy(self.p, a.ctypes.data, 8 * self.n, 1) == 0
        return self

    def numpy(self):
        out = np.empty(self.n)
        assert self._hip.hipMemcpy(out.ctypes.data, self.p, 8 * self.n, 2) == 0
        return out

    def __del__(self):
        try:
            self._hip.hipFree(self.p)
        except Exception:
            pass


def _fitted(w, **opts):
    from pybo_amd._lib import Engine
    e = Engine(0)
    for name, v in opts.items():
        e.set_option(name, v)
    e.fit(w['X'], w['y'], w['kernel'], w['ell'], w['rho'], w['sn2'], w['bias'])
    return e


def _dev(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return _DevBuf(a.size).put(a)


def _all_values(e, acq, param, dZ, M):
    """The d_acq-requesting call: every candidate's exact value (this call never prunes)."""
    buf = _DevBuf(M)
    e.sweep_dev(acq, param, dZ.data_ptr(), M, 0, d_acq=buf.data_ptr())
    e.sync()
    return buf.numpy()


def _topk_of(vals, k):
    idx = gp_ref.topk_desc(vals, k)
    return vals[idx], idx


def _flop_share(e, w, M):
    t = e.timers(reset=True)
    return t['sweep_trmm_flop'] / (float(w['N']) ** 2 * M), t


def _small(N, d, M, seed=0, kernel='se'):
    X, y, ell = synth_problem(N, d, seed=seed)
    rng = np.random.RandomState(seed + 100)
    return dict(X=X, y=y, ell=ell, rho=1.3, sn2=1e-3, bias=0.2, kernel=kernel, N=N, d=d, Xc=rng.rand(M, d))


def _compare_paths(w, M, ks=KS, host_form=True):
    """prune = 0 against prune = 1 against the top-k of the values of a d_acq-requesting call, device and host form."""
    e = _fitted(w)
    _, target = e.mean_at_obs()
    Z = w['Xc'][:M]
    dZ = _dev(Z)
    vals = _all_values(e, 'ei', target, dZ, M)
    shares = {}
    for k in ks:
        want_v, want_i = _topk_of(vals, k)
        got = {}
        for p in (0, 1):
            e.set_option('prune', p)
            e.timers(reset=True)
            got[p] = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
            shares[(k, p)] = _flop_share(e, w, M)[0]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), k
        assert np.array_equal(got[1][0], want_v) and np.array_equal(got[1][1], want_i), k
        if host_form and k in (10, 4096):
            r = e.sweep('ei', target, Z, k=k, want_all=False)
            assert np.array_equal(r['top_val'], want_v) and np.array_equal(r['top_idx'], want_i), k
    e.close()
    return shares


@pytest.mark.parametrize('name', ['ns', 'ns2', 'b'])
def test_pruned_and_plain_paths_agree_bit_for_bit_at_full_size(name):
    M = 1 << 20
    w = bench.make_workload(name, M)
    shares = _compare_paths(w, M)
    print(name, {k: '%.4f' % v for k, v in shares.items()})
    for k in KS:
        assert shares[(k, 0)] == 1.0


@pytest.mark.parametrize('N,d,M', [(1000, 3, 40000), (2049, 8, 33333), (300, 2, 13001)])
def test_pruned_and_plain_paths_agree_at_sizes_off_the_tile_grid(N, d, M):
    _compare_paths(_small(N, d, M, seed=N), M)


def test_two_shards_merged_equal_the_single_sweep():
    """The multi-rank path: each rank sweeps its contiguous shard (local indices + offset) and the k best pairs are
    merged value descending, index ascending."""
    M, k = 1 << 18, 10
    w = bench.make_workload('ns', M)
    e = _fitted(w)
    _, target = e.mean_at_obs()
    dZ = _dev(w['Xc'])
    e.set_option('prune', 0)
    whole = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    e.set_option('prune', 1)
    half = M // 2
    parts = []
    for r in range(2):
        dS = _dev(w['Xc'][r * half:(r + 1) * half])
        tv, ti = e.sweep_dev('ei', target, dS.data_ptr(), half, k)
        parts.append((tv, ti + r * half))
    v = np.concatenate([p[0] for p in parts])
    i = np.concatenate([p[1] for p in parts])
    order = np.lexsort((i, -v))[:k]
    assert np.array_equal(v[order], whole[0]) and np.array_equal(i[order], whole[1])
    e.close()


def test_a_candidate_s_value_does_not_depend_on_its_column_slot():
    """What compaction adds to the chunk / tile-order independence of DESIGN.md section 2: the exact chain on a permuted
    copy of the candidates returns, per candidate, the bits of the unpermuted run (values, means and variances)."""
    M = 20000 + 77
    for w in (_small(1500, 5, M, seed=4), _small(700, 8, M, seed=5, kernel='matern5')):
        e = _fitted(w)
        _, target = e.mean_at_obs()
        perm = np.random.RandomState(9).permutation(M)
        outs = []
        for Z in (w['Xc'], w['Xc'][perm]):
            dZ = _dev(Z)
            buf = _DevBuf(3 * M)
            e.sweep_dev('ei', target, dZ.data_ptr(), M, 0, d_acq=buf.at(0), d_mu=buf.at(M), d_s2=buf.at(2 * M))
            e.sync()
            outs.append(buf.numpy().reshape(3, M))
        assert np.array_equal(outs[0][:, perm], outs[1])
        e.close()


def test_edge_inputs():
    M, k = 50000, 10
    w = _small(1300, 4, M, seed=7)
    Z = w['Xc'].copy()
    e = _fitted(w)
    _, target = e.mean_at_obs()

    def both(Zc, tgt, kk=k, acq='ei'):
        dZ = _dev(Zc)
        vals = _all_values(e, acq, tgt, dZ, len(Zc))
        res = {}
        for p in (0, 1):
            e.set_option('prune', p)
            e.timers(reset=True)
            tv, ti = e.sweep_dev(acq, tgt, dZ.data_ptr(), len(Zc), kk)
            res[p] = (tv, ti, _flop_share(e, w, len(Zc))[0])
        assert np.array_equal(res[0][0], res[1][0], equal_nan=True) and np.array_equal(res[0][1], res[1][1])
        return vals, res

    # duplicated candidates at the top: ties resolved by index, as before
    vals, _ = both(Z, target)
    best = gp_ref.topk_desc(vals, 3)
    Zd = Z.copy()
    Zd[[40000, 17, 29999]] = Z[best[0]]
    Zd[[123, 45000]] = Z[best[1]]
    vals, res = both(Zd, target)
    want_v, want_i = _topk_of(vals, k)
    assert np.array_equal(res[1][0], want_v) and np.array_equal(res[1][1], want_i)
    assert set([17, 29999, 40000, int(best[0])]) == set(int(i) for i in res[1][1][:4])
    # a NaN coordinate: ranks last, everything else as before
    Zn = Z.copy()
    Zn[best[0], 1] = np.nan
    Zn[31000, 0] = np.nan
    vals, res = both(Zn, target)
    assert np.isnan(vals[best[0]]) and int(best[0]) not in res[1][1]
    clean = np.where(np.isnan(vals), -np.inf, vals)
    assert np.array_equal(res[1][1], gp_ref.topk_desc(clean, k))
    # a target so high that every EI underflows to 0: tau = 0, nothing is pruned, the plain loop runs (share 1 + the seeds)
    vals, res = both(Z, target + 1e6)
    assert np.all(vals == 0.0) and np.array_equal(res[1][1], np.arange(k)) and res[1][2] >= 1.0
    # M below the floor of the automatic rule: the plain path, exactly all the work
    e.set_option('prune', -1)
    e.timers(reset=True)
    dZ = _dev(Z[:20000])
    e.sweep_dev('ei', target, dZ.data_ptr(), 20000, k)
    assert _flop_share(e, w, 20000)[0] == 1.0
    # prune = 1 with UCB: the plain path
    vals, res = both(Z, 2.0, acq='ucb')
    assert res[1][2] == 1.0 and np.array_equal(res[1][1], gp_ref.topk_desc(vals, k))
    # sweep_cache = 1: the plain path (the cache needs every candidate's sums), and the warm step works afterwards
    e.set_option('prune', 1)
    e.set_option('sweep_cache', 1)
    e.timers(reset=True)
    dZ = _dev(Z)
    tv, ti = e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
    assert _flop_share(e, w, M)[0] == 1.0 and e.sweep_cache_size() == M
    xnew = Z[int(ti[0])]
    assert e.append(xnew, float(w['y'].max()))
    _, t2 = e.mean_at_obs()
    r = e.sweep_update('ei', t2, k=k, want_all=True)
    assert np.array_equal(r['top_idx'], gp_ref.topk_desc(r['acq'], k))
    e.close()


def test_the_work_really_goes_away_on_the_north_star_and_the_gate_declines_config_b():
    """A count, not a time: after one selection-only sweep of 'ns' under the default rule the sweep kernel's
    algorithmic flop are at most 3 % of N^2 M (0.9 % survivors + the seeds + the gate's generation, by the CPU count
    in DESIGN.md section 2.1); on config B, where the prior variance bounds nothing, the gate declines and they are
    exactly N^2 M."""
    M = 1 << 20
    for name, k in (('ns', 10), ('b', 10)):
        w = bench.make_workload(name, M)
        e = _fitted(w)
        _, target = e.mean_at_obs()
        dZ = _dev(w['Xc'])
        e.timers(reset=True)
        e.sweep_dev('ei', target, dZ.data_ptr(), M, k)
        share, t = _flop_share(e, w, M)
        print('%s: share of N^2 M evaluated exactly %.5f, launches %d, bound pass %.2f ms' %
              (name, share, t['sweep_trmm_launches'], t['sweep_bound']))
        if name == 'ns':
            assert share <= 0.03
            assert t['sweep_bound'] > 0
        else:
            assert share == 1.0
            assert t['sweep_bound'] == 0
        e.close()
