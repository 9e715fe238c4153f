"""
ctypes binding of libgpx.so (include/gpx.h).  This is the ONLY way pybo_amd reaches the GP arithmetic:
there is no CPU fallback -- if the shared library is missing, or no HIP device is present, the first use
raises.  (The CPU restatement under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

import numpy as np

# A handle owns up to four HIP streams (its own + three side streams: the factorisation's lookahead, and the correction
# pass of an ANNOUNCED observation that runs beside the recommender's calls).  ROCm multiplexes a process's streams onto
# GPU_MAX_HW_QUEUES hardware queues, 4 by default: with a second live handle (an ensemble, a second model, torch's own
# streams) two streams of one handle can land on the same queue and what was meant to overlap runs back to back --
# measured: the warm plug-in iteration 14.0 -> 16.3 ms at N = 8192 merely because another handle existed
# (profiles/history/).  Eight queues keep two handles apart.  The variable is read by the HIP runtime when it
# initialises, so it is the APPLICATION's to set (bench.py does, before importing torch): a
# library import does not change its host's environment -- see hw_queues_hint() below.


def hw_queues_hint():
    """None, or a one-line warning when this process runs several device handles on the runtime's default of 4 hardware
    queues (GPU_MAX_HW_QUEUES unset or < 8): streams meant to overlap may then share a queue."""
    try:
        q = int(os.environ.get('GPU_MAX_HW_QUEUES', '4'))
    except ValueError:
        q = 4
    if q >= 8:
        return None
    return ('pybo_amd: several device handles on GPU_MAX_HW_QUEUES=%d hardware queues; export GPU_MAX_HW_QUEUES=8 before '
            'the HIP runtime starts to keep their streams apart (see INTEGRATION.md)' % q)


_HERE = os.path.dirname(os.path.abspath(__file__))
# libgpx.so is the shipping library.  GPX_DIAGNOSTICS=1 selects libgpx_diag.so (the same objects, gpx_set_option also accepts the
# diagnostic knobs of csrc/gpx_diag.h: what the test-suite and the A/B scripts drive); GPX_LIB_PATH: any other build of the ABI.
LIB_PATH = os.environ.get('GPX_LIB_PATH') or os.path.join(
    _HERE, 'csrc', 'libgpx_diag.so' if os.environ.get('GPX_DIAGNOSTICS', '0') not in ('', '0') else 'libgpx.so')

# every symbol include/gpx.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int64)
_i64 = C.c_int64
_dbl = C.c_double
# every symbol pybo_amd/csrc/gpx_diag.h declares (exported by both builds)
DIAG_SYMBOLS = {
    'gpx_chol_trace': (_i64, [_P, _P, _i64]),
    'gpx_chol_tasks2': (_i64, [C.c_int, C.c_int, _P, _i64, _P]),
    'gpx_prune_report': (C.c_int, [_P, _P, C.c_int, _P, _P, _i64, _P, _P, _i64]),
    'gpx_prune_dots': (C.c_int, [_P, _P]),
    'gpx_prune_rows': (C.c_int, [_P, _P, _P, _P, _i64]),
    'gpx_ensemble_prune_report': (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _i64]),
    'gpx_constrained_prune_report': (C.c_int, [_P, _P, C.c_int, _P, _P, _i64]),
}
SYMBOLS = {
    'gpx_create': (C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    'gpx_destroy': (C.c_int, [_P]),
    'gpx_last_error': (C.c_char_p, [_P]),
    'gpx_version': (C.c_int, []),
    'gpx_set_option': (C.c_int, [_P, C.c_char_p, _i64]),
    'gpx_fit': (C.c_int, [_P, _P, _i64, _i64, _P, C.c_int, _P, _dbl, _dbl, _dbl]),
    'gpx_fit_dev': (C.c_int, [_P, _P, _i64, _i64, _P, C.c_int, _P, _dbl, _dbl, _dbl]),
    'gpx_loglik': (C.c_int, [_P, _P]),
    'gpx_loglik_batch': (C.c_int, [_P, _i64, _P, _P]),
    'gpx_loglik_grad': (C.c_int, [_P, _P, _P]),
    'gpx_append': (C.c_int, [_P, _P, _dbl]),
    'gpx_append_begin': (C.c_int, [_P, _P]),
    'gpx_fail_pivot': (_i64, [_P]),
    'gpx_get_matrix': (C.c_int, [_P, C.c_int, _P]),
    'gpx_get_vectors': (C.c_int, [_P, _P, _P]),
    'gpx_fit_stage': (C.c_int, [_P, _P, _i64, _i64, _P, C.c_int, _P, _dbl, _dbl, _dbl, C.c_int]),
    'gpx_mean_at_obs': (C.c_int, [_P, _P, _P]),
    'gpx_var_at_obs': (C.c_int, [_P, _P]),
    'gpx_capacity': (_i64, [_P]),
    'gpx_predict': (C.c_int, [_P, _P, _i64, _P, _P, _P, _P]),
    'gpx_predict_mean': (C.c_int, [_P, _P, _i64, _P, _P]),
    'gpx_predict_cov': (C.c_int, [_P, _P, _i64, _P, _P]),
    'gpx_sample_joint': (C.c_int, [_P, _P, _i64, _P, _i64, C.c_int, _dbl, _P]),
    'gpx_sweep': (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _i64, _i64, _P, _P, _P, _P, _P]),
    'gpx_sweep_dev': (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _i64, _i64, _P, _P, _P, _P, _P]),
    'gpx_sweep_update': (C.c_int, [_P, C.c_int, _P, C.c_int, _i64, _P, _P, _P, _P, _P]),
    'gpx_sweep_update_dev': (C.c_int, [_P, C.c_int, _P, C.c_int, _i64, _P, _P, _P, _P, _P]),
    'gpx_sweep_batch': (C.c_int, [_P, C.c_int, _P, C.c_int, _i64, _P, _P, _P, _P]),
    'gpx_sweep_batch_fantasy': (C.c_int, [_P, C.c_int, _P, C.c_int, _i64, _P, _i64, _i64, C.c_int, _P, _i64, _P, _P, _P, _P]),
    'gpx_sweep_cache_size': (_i64, [_P]),
    'gpx_kg_grad': (C.c_int, [_P, _P, _i64, _P, _i64, _P, _P]),
    'gpx_rff_sweep': (C.c_int, [_P, _P, _P, _P, _i64, _i64, _i64, _dbl, _P, _i64, _i64, _P, _P, _P]),
    'gpx_rff_sweep_dev': (C.c_int, [_P, _P, _P, _P, _i64, _i64, _i64, _dbl, _P, _i64, _i64, _P, _P, _P]),
    'gpx_rff_grad': (C.c_int, [_P, _P, _P, _P, _i64, _i64, _dbl, _P, _i64, _P, _P]),
    'gpx_rff_gram': (C.c_int, [_P, _P, _P, _i64, _P, _P]),
    'gpx_rff_gram_batch': (C.c_int, [_P, _P, _P, _i64, _i64, _P, _P]),
    'gpx_rff_posterior': (C.c_int, [_P, _P, _P, _P, _i64, _i64, _dbl, _P]),
    'gpx_path_weights': (C.c_int, [_P, _P, _P, _P, _P, _i64, _i64, _dbl, _P, _P]),
    'gpx_path_sweep': (C.c_int, [_P, _P, _P, _P, _P, _i64, _i64, _i64, _i64, _dbl, _P, _i64, _i64, _P, _P, _P]),
    'gpx_path_sweep_dev': (C.c_int, [_P, _P, _P, _P, _P, _i64, _i64, _i64, _i64, _dbl, _P, _i64, _i64, _P, _P, _P]),
    'gpx_path_grad': (C.c_int, [_P, _P, _P, _P, _P, _i64, _i64, _i64, _dbl, _P, _i64, _P, _P]),
    'gpx_ensemble_sweep': (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _i64, _i64, _P, _P, _P, _P, _P]),
    'gpx_ensemble_sweep_dev': (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _i64, _i64, _P, _P, _P, _P, _P]),
    'gpx_ensemble_sweep_batch': (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _i64, _P, _P, _P]),
    'gpx_ensemble_predict': (C.c_int, [_P, C.c_int, _P, _i64, _P, _P, _P, _P]),
    'gpx_constrained_sweep': (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, _P, _i64, _i64, _P, _P, _P, _P]),
    'gpx_constrained_sweep_dev': (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, _P, _i64, _i64, _P, _P, _P, _P]),
    'gpx_constrained_sweep_batch': (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, _i64, _P, _P, _P]),
    'gpx_ehvi_sweep': (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _i64, _i64, _P, _P, _P]),
    'gpx_ehvi_sweep_dev': (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _i64, _i64, _P, _P, _P, _P]),
    'gpx_ehvi_fold_dev': (C.c_int, [_P, _P, _i64, _P, C.c_int, _P, _i64, _P, _P, _P]),
    'gpx_ehvi_sweep_batch': (C.c_int, [_P, _P, _P, C.c_int, _P, _i64, _P, _P, _P, _P, _P]),
    'gpx_grid_create': (C.c_int, [C.c_int, C.c_int, _P, _i64, _i64, C.c_uint64, _i64, _P, C.c_int, C.POINTER(_P)]),
    'gpx_grid_data': (_P, [_P]),
    'gpx_grid_rows': (C.c_int, [_P, _P, _i64, _P]),
    'gpx_grid_destroy': (C.c_int, [_P]),
    'gpx_comm_unique_id': (C.c_int, [_P]),
    'gpx_comm_init': (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    'gpx_comm_destroy': (C.c_int, [_P]),
    'gpx_comm_size': (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'gpx_comm_last_error': (C.c_char_p, []),
    'gpx_topk_allgather': (C.c_int, [_P, _i64, _i64, _i64, _P, _P]),
    'gpx_timers': (C.c_int, [_P, _P, C.c_int, C.c_int]),
    'gpx_sync': (C.c_int, [_P]),
    'gpx_diagnostics': (C.c_int, []),
}

GPX_OK, GPX_EARG, GPX_ENOTPD, GPX_EHIP, GPX_EOOM, GPX_ESTATE, GPX_ERCCL = 0, -1, -2, -3, -4, -5, -6
COMM_ID_BYTES = 128
KERNELS = {'se': 0, 'matern5': 1, 'matern3': 2, 'matern1': 3}
ACQ = {'ei': 0, 'pi': 1, 'ucb': 2, 'mean': 3, 'mes': 16}       # (ids 4 .. 15 are refused by the library)
# The acquisitions that are NOT a function of a candidate's own moments, in a table of their own (tests/test_mes_cpu.py pins ACQ's
# values): 'kg', the knowledge gradient over a support set -- param = the set (m, d), m <= KG_MAX_SUPPORT; cold sweeps only; ids
# 17 .. 31 are refused by the library
ACQ_SUPPORT = {'kg': 32}
KG_MAX_SUPPORT = 127
TIMER_NAMES = ['gram', 'cholesky', 'trtri', 'alpha', 'cross_gram', 'sweep_trmm', 'acq_topk', 'rff',
               'sweep_trmm_launches', 'sweep_trmm_flop', 'copies', 'append', 'rank1', 'rff_sweep', 'rff_sweep_ops',
               'chol_fallbacks', 'sweep_sclk_mhz', 'rff_sclk_mhz', 'trtri_ahead', 'sweep_bound', 'batch', 'joint']
TOPK_MAX = 4096
JOINT_MAX = 4096     # points of a joint posterior (gpx_predict_cov / gpx_sample_joint)

_lib = None


def acq_id(acq):
    """The library's id of an acquisition given by name (ACQ, ACQ_SUPPORT) or by number."""
    if not isinstance(acq, str):
        return int(acq)
    return ACQ[acq] if acq in ACQ else ACQ_SUPPORT[acq]


def chol_tasks(nblocks, chunks=0):
    """The task lists of the task-graph factorisation (host only): two (n, 8) int16 arrays
    {type, I, J, k0, k1, ordinal, aux, reserved} -- the critical list and the workers' list (csrc/gpx_diag.h: gpx_chol_tasks2)."""
    lib = load()
    counts = np.zeros(2, dtype=np.int64)
    tot = lib.gpx_chol_tasks2(nblocks, chunks, None, 0, _ptr(counts))
    if tot < 0:
        raise ValueError('gpx_chol_tasks2: bad arguments')
    out = np.zeros((max(int(tot), 1), 8), dtype=np.int16)
    lib.gpx_chol_tasks2(nblocks, chunks, _ptr(out), int(tot), _ptr(counts))
    o = np.cumsum(np.r_[0, counts])
    return [out[o[q]:o[q + 1]] for q in range(2)]


class GpxError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, 'libgpx error %d: %s' % (code, msg))
        self.code = code


def load():
    """Load libgpx.so (once) and set the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError('pybo_amd: %s not found -- build it with `python __graft_entry__.py` '
                              '(or pybo_amd/csrc/build.sh); there is no CPU fallback.' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(DIAG_SYMBOLS.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _dptr(p):
    """A device pointer given as an integer (0 / None: NULL)."""
    return _P(p) if p else None


def _handles(engines):
    return (_P * len(engines))(*[e._h for e in engines])


def _topk_out(k, S=None):
    """The top-k buffers of a sweep entry ((S, k) for S draws) and the pointers it takes for them: NULL for k = 0."""
    shape = k if S is None else (S, k)
    tv, ti = np.empty(shape), np.empty(shape, dtype=np.int64)
    return tv, ti, _ptr(tv) if k else None, _ptr(ti) if k else None


def _candidates(Xc, d, **want):
    """(dev, pointer, M, outputs) of the candidates of a sweep entry with a host and a _dev form: a DeviceGrid gives its device pointer
    and no host output; anything else is a host array (M, d) and gives an (M,) buffer for every name of `want` that is true."""
    if isinstance(Xc, DeviceGrid):
        return True, Xc.ptr, len(Xc), dict.fromkeys(want)
    Xc = _f64(Xc).reshape(-1, d)      # (the pointer keeps the array alive)
    return False, _ptr(Xc), len(Xc), {name: np.empty(len(Xc)) if on else None for name, on in want.items()}


def _report_head(scal):
    """The eight scalars every prune report starts with."""
    r = {name: int(v) for name, v in zip(('path', 'M', 'k', 'G', 'Gg', 'done', 'cap', 'nsurv'), scal[:8])}
    r['path'] = Engine.PRUNE_PATHS[r['path']]
    return r


def _report_vectors(r, vectors, fetch):
    """The second call of a prune report, where the bound pass ran: r['ub'] (M,) and r['idx'] (the survivors; empty where it fell back),
    filled by fetch(ub pointer, idx pointer, nidx)."""
    if vectors and r['path'] in ('pruned', 'fell back'):
        nidx = r['nsurv'] if r['path'] == 'pruned' else 0
        r['ub'] = np.empty(r['M'])
        r['idx'] = np.empty(nidx, dtype=np.int64)
        fetch(_ptr(r['ub']), _ptr(r['idx']), nidx)
    return r


def _acq_params(param):
    """The (params, nparams) pair of a sweep entry from an acquisition parameter: a scalar (EI / PI target, UCB beta) or None (the
    mean) is one double; an array (the maximum samples of 'mes', (S,) or member-major (n, S)) passes through flattened, untouched."""
    if param is None or np.ndim(param) == 0:
        return _f64([0.0 if param is None else param]), 1
    params = _f64(param).reshape(-1)
    return params, len(params)


def sobol_direction_numbers(d, nbits):
    """Direction numbers (d, bits) uint32 of scipy's unscrambled Sobol' generator (Joe-Kuo), LSB-first in the
    Gray-code recurrence: point i = XOR_b [bit b of i^(i>>1)] * sv[:, b], x = point * 2^-bits.  Read from the
    generator object when it exposes them, otherwise derived through the public API (the point with Gray
    code 2^b is number 2^(b+1) - 1); checked against the generator's first points either way."""
    from scipy.stats import qmc
    eng = qmc.Sobol(d, scramble=False)
    bits = int(getattr(eng, 'bits', 30) or 30)
    sv = getattr(eng, '_sv', None)
    if sv is not None and np.shape(sv) == (d, bits):
        sv = np.ascontiguousarray(sv, dtype=np.uint32)
    else:
        sv = np.zeros((d, bits), dtype=np.uint32)
        pos = 0
        for b in range(min(bits, max(int(nbits), 4))):
            target = 2 ** (b + 1) - 1
            if target > pos:
                eng.fast_forward(target - pos)
            sv[:, b] = np.round(eng.random(1)[0] * 2.0 ** bits).astype(np.uint32)
            pos = target + 1
    ref = qmc.Sobol(d, scramble=False).random(16)
    acc = np.zeros(d, dtype=np.uint32)
    for i in range(16):
        g = i ^ (i >> 1)
        acc[:] = 0
        for b in range(5):
            if (g >> b) & 1:
                acc ^= sv[:, b]
        if not np.array_equal(acc * 2.0 ** -bits, ref[i]):
            raise RuntimeError('scipy Sobol generator does not follow the expected Gray-code recurrence')
    return sv, bits


class DeviceGrid(object):
    """A candidate grid generated and kept in HBM (gpx_grid_*): `kind` 'sobol' (points first..first+n-1 of
    scipy's unscrambled sequence, scaled to the box) or 'uniform' (Philox4x32-10 keyed by `seed`).  Behaves
    like a read-only (n, d) array for the solver: len(), .shape, grid[idx] (rows copied to the host),
    np.asarray(grid) (the whole grid -- avoid on the hot path)."""

    def __init__(self, kind, bounds, n, seed=0, first=0, device=0):
        self._lib = load()
        bounds = _f64(np.array(bounds, dtype=float, ndmin=2))
        n = int(n)
        d = len(bounds)
        g = _P()
        if kind == 'sobol':
            sv, bits = sobol_direction_numbers(d, int(first + n).bit_length())
            rc = self._lib.gpx_grid_create(int(device), 1, _ptr(bounds), n, d, 0, int(first),
                                           sv.ctypes.data_as(_P), bits, C.byref(g))
        elif kind == 'uniform':
            rc = self._lib.gpx_grid_create(int(device), 0, _ptr(bounds), n, d, int(seed), int(first), None, 0,
                                           C.byref(g))
        else:
            raise ValueError("grid kind must be 'sobol' or 'uniform'")
        if rc != GPX_OK:
            raise GpxError(rc, (self._lib.gpx_last_error(None) or b'').decode())
        self._g = g
        self.kind, self.bounds, self.device = kind, bounds, int(device)
        self.shape = (n, d)
        self.ptr = self._lib.gpx_grid_data(g)

    def __len__(self):
        return self.shape[0]

    def rows(self, idx):
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        out = np.empty((len(idx), self.shape[1]))
        rc = self._lib.gpx_grid_rows(self._g, _ptr(idx), len(idx), _ptr(out))
        if rc != GPX_OK:
            raise GpxError(rc, (self._lib.gpx_last_error(None) or b'').decode())
        return out

    def view(self, lo, hi):
        """Rows [lo, hi) as a grid of their own, without a copy; the same object for the same range (a model keys
        its warm sweep cache on the grid object it swept)."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= len(self):
            raise IndexError('grid view out of range')
        views = self.__dict__.setdefault('_views', {})
        if (lo, hi) not in views:
            views[(lo, hi)] = DeviceGridView(self, lo, hi)
        return views[(lo, hi)]

    def __getitem__(self, idx):
        if isinstance(idx, slice):                  # grid[lo:hi] (pybo_amd.dist shards a grid this way)
            lo, hi, step = idx.indices(len(self))
            if step == 1:
                return self.view(lo, max(lo, hi))   # contiguous: stays on the device
            return self.rows(np.arange(lo, hi, step, dtype=np.int64))
        if np.isscalar(idx):
            return self.rows([idx])[0]
        return self.rows(idx)

    def __array__(self, dtype=None, copy=None):
        out = np.empty(self.shape)
        rc = self._lib.gpx_grid_rows(self._g, None, 0, _ptr(out))
        if rc != GPX_OK:
            raise GpxError(rc, (self._lib.gpx_last_error(None) or b'').decode())
        return out if dtype is None else out.astype(dtype)

    def close(self):
        if getattr(self, '_g', None):
            self._lib.gpx_grid_destroy(self._g)
            self._g = None
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGridView(DeviceGrid):
    """Rows [lo, hi) of a DeviceGrid as a grid of their own (no copy: a pointer into the parent's HBM array) -- what
    a rank of the multi-process layout sweeps when every rank holds the whole grid (pybo_amd.dist.sharded_topk)."""

    def __init__(self, parent, lo, hi):
        self._lib = parent._lib
        self._parent, self._lo = parent, int(lo)
        self._g = None
        self.kind, self.bounds, self.device = parent.kind, parent.bounds, parent.device
        self.shape = (int(hi) - int(lo), parent.shape[1])
        self.ptr = parent.ptr + int(lo) * parent.shape[1] * 8

    def rows(self, idx):
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError('grid row out of range')
        return self._parent.rows(idx + self._lo)

    def __array__(self, dtype=None, copy=None):
        out = self._parent.rows(np.arange(self._lo, self._lo + len(self), dtype=np.int64))
        return out if dtype is None else out.astype(dtype)

    def close(self):
        self.ptr = None


class ShardedDeviceGrid(object):
    """ONE logical (n, d) grid laid out over several devices for pybo_amd.models.ShardedGP: shard p = rows
    shard_bounds(n, p, P) generated and kept on devices[p] (Sobol': the same points of the sequence; uniform: the same
    Philox stream -- the concatenation of the shards IS the single-device grid, bit for bit).  Behaves like a
    read-only (n, d) array for the solver: len(), .shape, grid[idx] (rows fetched from their owners)."""

    def __init__(self, kind, bounds, n, devices, seed=0, first=0):
        n, devices = int(n), [int(dv) for dv in devices]
        P = len(devices)
        self.kind, self.devices = kind, devices
        self.shards = []
        for p, dv in enumerate(devices):
            lo, hi = (n * p) // P, (n * (p + 1)) // P
            g = DeviceGrid(kind, bounds, hi - lo, seed=seed, first=int(first) + lo, device=dv) if hi > lo else None
            self.shards.append((lo, hi, g))
        self.bounds = np.array(bounds, dtype=float, ndmin=2)
        self.shape = (n, len(self.bounds))

    def __len__(self):
        return self.shape[0]

    def rows(self, idx):
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        out = np.empty((len(idx), self.shape[1]))
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError('grid row out of range')
        for lo, hi, g in self.shards:
            mine = np.flatnonzero((idx >= lo) & (idx < hi))
            if len(mine):
                out[mine] = g.rows(idx[mine] - lo)
        return out

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            return self.rows(np.arange(*idx.indices(len(self)), dtype=np.int64))
        if np.isscalar(idx):
            return self.rows([idx])[0]
        return self.rows(idx)

    def __array__(self, dtype=None, copy=None):
        out = np.concatenate([np.asarray(g) for _, _, g in self.shards if g is not None])
        return out if dtype is None else out.astype(dtype)

    def close(self):
        for _, _, g in self.shards:
            if g is not None:
                g.close()


class Comm(object):
    """RCCL communicator bound to an Engine's device and stream (gpx_comm_*): the exchange step of the sharded
    sweep without torch.distributed.  Rank 0 creates the id with `Comm.unique_id()` and hands the 128 bytes to
    the other ranks over any side channel; every rank then constructs `Comm(engine, rank, nranks, id)`."""

    @staticmethod
    def unique_id():
        lib = load()
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        rc = lib.gpx_comm_unique_id(C.cast(buf, _P))
        if rc != GPX_OK:
            raise GpxError(rc, (lib.gpx_comm_last_error() or b'').decode())
        return bytes(buf)

    def __init__(self, engine, rank, nranks, uid):
        self._lib = load()
        if len(uid) != COMM_ID_BYTES:
            raise ValueError('the communicator id has %d bytes' % COMM_ID_BYTES)
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
        c = _P()
        rc = self._lib.gpx_comm_init(engine._h, int(rank), int(nranks), C.cast(buf, _P), C.byref(c))
        if rc != GPX_OK:
            raise GpxError(rc, (self._lib.gpx_comm_last_error() or b'').decode())
        self._c, self._engine = c, engine            # the engine must outlive the communicator
        self.rank, self.nranks = int(rank), int(nranks)

    def topk_allgather(self, n, index_offset, k):
        """Gather the engine's last n device (value, index) pairs from every rank; k > 0: merged k best
        (identical on every rank), k = 0: all nranks*n pairs in rank order."""
        m = int(k) if k > 0 else int(n) * self.nranks
        tv = np.empty(m)
        ti = np.empty(m, dtype=np.int64)
        rc = self._lib.gpx_topk_allgather(self._c, int(n), int(index_offset), int(k), _ptr(tv), _ptr(ti))
        if rc != GPX_OK:
            raise GpxError(rc, (self._lib.gpx_comm_last_error() or b'').decode())
        return tv, ti

    def close(self):
        if getattr(self, '_c', None):
            self._lib.gpx_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(object):
    """One gpx handle = one (device, model).  Thin, stateless-in-Python wrapper over the C-ABI."""

    def __init__(self, device=0, stream=None):
        self._lib = load()
        h = _P()
        rc = self._lib.gpx_create(int(device), _P(stream) if stream else None, C.byref(h))
        if rc != GPX_OK:
            raise GpxError(rc, (self._lib.gpx_last_error(None) or b'').decode())
        self._h = h
        self.device = int(device)
        self.N = 0
        self.d = 0
        Engine._live += 1
        if Engine._live > 1 and not Engine._hinted:
            hint = hw_queues_hint()
            Engine._hinted = True
            if hint:
                import warnings
                warnings.warn(hint, RuntimeWarning, stacklevel=2)

    _live = 0            # handles alive in this process
    _hinted = False      # the GPU_MAX_HW_QUEUES hint is given once

    def close(self):
        if getattr(self, '_h', None):
            self._lib.gpx_destroy(self._h)
            self._h = None
            Engine._live -= 1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != GPX_OK:
            msg = (self._lib.gpx_last_error(self._h) or b'').decode()
            if rc == GPX_ENOTPD:
                raise np.linalg.LinAlgError(msg)
            raise GpxError(rc, msg)

    def set_option(self, name, value):
        self._check(self._lib.gpx_set_option(self._h, name.encode(), int(value)))

    # -- fit -----------------------------------------------------------------------------------
    def fit(self, X, y, kernel, ell, rho, sn2, bias, stage=3):
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError('X must be (N, d)')
        y = _f64(y).reshape(-1)
        N, d = X.shape
        if len(y) != N:
            raise ValueError('X and y disagree on N')
        ell = _f64(np.broadcast_to(np.asarray(ell, dtype=float), (d,)))
        kid = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        self.N, self.d = N, d
        if stage == 3:
            rc = self._lib.gpx_fit(self._h, _ptr(X), N, d, _ptr(y), kid, _ptr(ell), rho, sn2, bias)
        else:
            rc = self._lib.gpx_fit_stage(self._h, _ptr(X), N, d, _ptr(y), kid, _ptr(ell), rho, sn2, bias,
                                         int(stage))
        self._check(rc)
        self.N, self.d = N, d

    def fit_dev(self, dX_ptr, N, d, dy_ptr, kernel, ell, rho, sn2, bias):
        ell = _f64(np.broadcast_to(np.asarray(ell, dtype=float), (d,)))
        kid = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        self._check(self._lib.gpx_fit_dev(self._h, _P(dX_ptr), N, d, _P(dy_ptr), kid, _ptr(ell), rho, sn2,
                                          bias))
        self.N, self.d = N, d

    def loglik(self):
        out = C.c_double()
        self._check(self._lib.gpx_loglik(self._h, C.byref(out)))
        return out.value

    def loglik_batch(self, hypers):
        """log p(y | X, theta_b) for B hyper-parameter vectors [sn2, rho, ell_1..d, bias] on the resident data: one
        batched launch chain, one synchronisation; the engine's own fit is untouched."""
        hypers = _f64(hypers).reshape(-1, self.d + 3)
        out = np.empty(len(hypers))
        self._check(self._lib.gpx_loglik_batch(self._h, len(hypers), _ptr(hypers), _ptr(out)))
        return out

    def loglik_grad(self):
        """(L, dL/d[sn2, rho, ell_1..d, bias]) of the current fit in NATURAL parameters (gpx_loglik_grad): L is gpx_loglik's value,
        the gradient comes from one triangular product on the device."""
        out = C.c_double()
        grad = np.empty(self.d + 3)
        self._check(self._lib.gpx_loglik_grad(self._h, C.byref(out), _ptr(grad)))
        return out.value, grad

    def append(self, x, y):
        """Rank-1 extension by one observation; returns False when a refit is needed (block boundary)."""
        x = _f64(x).reshape(-1)
        if len(x) != self.d:
            raise ValueError('x must have %d coordinates' % self.d)
        rc = self._lib.gpx_append(self._h, _ptr(x), float(y))
        if rc == GPX_ESTATE:
            return False
        self._check(rc)
        self.N += 1
        return True

    def append_begin(self, x):
        """Announce the next observation's location (gpx_append_begin): the value-independent work of the coming
        append runs ahead.  Returns False when there is nothing to run ahead (no live sweep cache, block boundary)."""
        x = _f64(x).reshape(-1)
        if len(x) != self.d:
            raise ValueError('x must have %d coordinates' % self.d)
        rc = self._lib.gpx_append_begin(self._h, _ptr(x))
        if rc == GPX_ESTATE:
            return False
        self._check(rc)
        return True

    def fail_pivot(self):
        return int(self._lib.gpx_fail_pivot(self._h))

    def get_matrix(self, which):
        out = np.empty((self.N, self.N))
        self._check(self._lib.gpx_get_matrix(self._h, {'L': 0, 'T': 1, 'K': 2}[which], _ptr(out)))
        return out

    def get_vectors(self):
        a = np.empty(self.N)
        alpha = np.empty(self.N)
        self._check(self._lib.gpx_get_vectors(self._h, _ptr(a), _ptr(alpha)))
        return a, alpha

    def mean_at_obs(self):
        mu = np.empty(self.N)
        mx = C.c_double()
        self._check(self._lib.gpx_mean_at_obs(self._h, _ptr(mu), C.byref(mx)))
        return mu, mx.value

    def var_at_obs(self):
        s2 = np.empty(self.N)
        self._check(self._lib.gpx_var_at_obs(self._h, _ptr(s2)))
        return s2

    def capacity(self):
        """Rows the handle's factor buffers are allocated for (they stay allocated until the handle is closed)."""
        return int(self._lib.gpx_capacity(self._h))

    # -- posterior / sweep -----------------------------------------------------------------------
    def predict(self, Xc, grad=False):
        Xc = _f64(Xc).reshape(-1, self.d)
        M = len(Xc)
        mu = np.empty(M)
        s2 = np.empty(M)
        if grad:
            dmu = np.empty((M, self.d))
            ds2 = np.empty((M, self.d))
            self._check(self._lib.gpx_predict(self._h, _ptr(Xc), M, _ptr(mu), _ptr(s2), _ptr(dmu), _ptr(ds2)))
            return mu, s2, dmu, ds2
        self._check(self._lib.gpx_predict(self._h, _ptr(Xc), M, _ptr(mu), _ptr(s2), None, None))
        return mu, s2

    def predict_mean(self, Xc, grad=False):
        """Posterior mean [and its gradient] only, k(x, X).alpha: no pass over the factor's inverse per call."""
        Xc = _f64(Xc).reshape(-1, self.d)
        M = len(Xc)
        mu = np.empty(M)
        dmu = np.empty((M, self.d)) if grad else None
        self._check(self._lib.gpx_predict_mean(self._h, _ptr(Xc), M, _ptr(mu), _ptr(dmu) if grad else None))
        return (mu, dmu) if grad else mu

    def predict_cov(self, Xc):
        """Joint latent posterior at the rows of Xc (at most JOINT_MAX): (mu (M,), cov (M, M)), cov = k(Z, Z) - V^T V raw and symmetric
        bit for bit (gpx_predict_cov)."""
        Xc = _f64(Xc).reshape(-1, self.d)
        M = len(Xc)
        mu = np.empty(M)
        cov = np.empty((M, M))
        self._check(self._lib.gpx_predict_cov(self._h, _ptr(Xc), M, _ptr(mu), _ptr(cov)))
        return mu, cov

    def kg_grad(self, A, Xc):
        """Knowledge gradient over the support set A (m, d), m <= KG_MAX_SUPPORT, and its gradient at the rows of Xc (at most JOINT_MAX):
        (f (M,), g (M, d)) (gpx_kg_grad); f agrees with sweep('kg', A, Xc) to rounding."""
        A = _f64(A).reshape(-1, self.d)
        Xc = _f64(Xc).reshape(-1, self.d)
        M = len(Xc)
        f = np.empty(M)
        g = np.empty((M, self.d))
        self._check(self._lib.gpx_kg_grad(self._h, _ptr(A), len(A), _ptr(Xc), M, _ptr(f), _ptr(g)))
        return f, g

    def sample_joint(self, Xc, z, noisy=False, jitter=0.0):
        """Joint draws at the rows of Xc from the standard normals z (S, M): out[s] = mu + R^T z[s] with R^T R = cov + (noisy ? sn2 : 0) I
        + jitter I, factored on the device (gpx_sample_joint); LinAlgError when that matrix is not positive definite."""
        Xc = _f64(Xc).reshape(-1, self.d)
        M = len(Xc)
        z = _f64(z).reshape(-1, M)
        out = np.empty(z.shape)
        self._check(self._lib.gpx_sample_joint(self._h, _ptr(Xc), M, _ptr(z), len(z), int(bool(noisy)), float(jitter), _ptr(out)))
        return out

    def sweep(self, acq, param, Xc, k=0, want_all=True, want_moments=False):
        """Host-buffer sweep.  Returns dict(top_val, top_idx, acq, mu, s2)."""
        Xc = _f64(Xc)
        Xc = Xc.reshape(-1, self.d) if self.d else np.atleast_2d(Xc)
        M = len(Xc)
        params, nparams = _acq_params(param)
        tv, ti, ptv, pti = _topk_out(k)
        out = np.empty(M) if want_all else None
        mu = np.empty(M) if want_moments else None
        s2 = np.empty(M) if want_moments else None
        self._check(self._lib.gpx_sweep(self._h, acq_id(acq), _ptr(params), nparams, _ptr(Xc), M, k, ptv, pti, _ptr(out), _ptr(mu), _ptr(s2)))
        return dict(top_val=tv, top_idx=ti, acq=out, mu=mu, s2=s2)

    def sweep_update(self, acq, param, k=0, want_all=True, want_moments=False):
        """Re-score the cached candidate set (option sweep_cache, kept current by append): O(M)."""
        M = self.sweep_cache_size()
        params, nparams = _acq_params(param)
        tv, ti, ptv, pti = _topk_out(k)
        out = np.empty(M) if want_all else None
        mu = np.empty(M) if want_moments else None
        s2 = np.empty(M) if want_moments else None
        self._check(self._lib.gpx_sweep_update(self._h, acq_id(acq), _ptr(params), nparams, k, ptv, pti, _ptr(out), _ptr(mu), _ptr(s2)))
        return dict(top_val=tv, top_idx=ti, acq=out, mu=mu, s2=s2)

    def sweep_cache_size(self):
        return int(self._lib.gpx_sweep_cache_size(self._h))

    def _batch_out(self, nb, want_s2_all):
        """The result of a single-model batch entry, for the library to fill: dict(sel_val, sel_idx, sel_s2[, s2_all])."""
        n = max(int(nb), 0)
        out = dict(sel_val=np.empty(n), sel_idx=np.empty(n, dtype=np.int64), sel_s2=np.empty(n))
        if want_s2_all:
            out['s2_all'] = np.empty(self.sweep_cache_size())
        return out

    def sweep_batch(self, kind, param, nb, want_s2_all=False):
        """nb greedy picks on the live sweep cache (gpx_sweep_batch), each conditioned on the earlier ones at their posterior
        mean.  Returns dict(sel_val, sel_idx, sel_s2[, s2_all]); model, cache and a pending announcement are untouched."""
        aid = acq_id(kind)
        params, nparams = _acq_params(param)
        out = self._batch_out(nb, want_s2_all)
        self._check(self._lib.gpx_sweep_batch(self._h, aid, _ptr(params), nparams, int(nb), _ptr(out['sel_val']), _ptr(out['sel_idx']),
                                              _ptr(out['sel_s2']), _ptr(out.get('s2_all'))))
        return out

    def sweep_batch_fantasy(self, kind, param, nb, eps, incumbent=1, pending=None, want_s2_all=False):
        """nb greedy picks on the live sweep cache with the pending outcomes integrated out over the S = len(eps) joint fantasies
        (gpx_sweep_batch_fantasy): `eps` (S, >= nb - 1) standard normals, row s the innovations of fantasy s in pick order;
        `incumbent` 1: every fantasy's EI / PI target follows its own fantasised observations, 0: it stays at `param`; `pending`:
        cache rows already being evaluated, which the leading rounds are forced to.  Returns dict(sel_val, sel_idx, sel_s2[, s2_all])."""
        aid = acq_id(kind)
        params, nparams = _acq_params(param)
        eps = _f64(eps)
        if eps.ndim != 2:
            raise ValueError('eps must be a (S, >= nb - 1) array')
        pend = None if pending is None else np.ascontiguousarray(pending, dtype=np.int64).reshape(-1)
        out = self._batch_out(nb, want_s2_all)
        self._check(self._lib.gpx_sweep_batch_fantasy(self._h, aid, _ptr(params), nparams, int(nb), _ptr(eps), eps.shape[0], eps.shape[1],
                                                      int(incumbent), _ptr(pend), 0 if pend is None else len(pend), _ptr(out['sel_val']),
                                                      _ptr(out['sel_idx']), _ptr(out['sel_s2']), _ptr(out.get('s2_all'))))
        return out

    def sweep_dev(self, acq, param, dXc_ptr, M, k, d_acq=None, d_mu=None, d_s2=None):
        params, nparams = _acq_params(param)
        tv, ti, ptv, pti = _topk_out(k)
        self._check(self._lib.gpx_sweep_dev(self._h, acq_id(acq), _ptr(params), nparams, _P(dXc_ptr), M, k, ptv, pti, _dptr(d_acq), _dptr(d_mu),
                                            _dptr(d_s2)))
        return tv, ti

    @staticmethod
    def ensemble_sweep(engines, acq, param, Xc, k=0, want_all=True, want_moments=False):
        """Hyper-parameter ensemble sweep (gpx_ensemble_sweep[_dev]): the member sweeps and their average stay
        on the device.  `Xc`: host array (M, d) or a DeviceGrid.  Returns dict(top_val, top_idx, acq, mu, s2)."""
        lead = engines[0]
        params, nparams = _acq_params(param)
        tv, ti, ptv, pti = _topk_out(k)
        dev, X, M, o = _candidates(Xc, lead.d, acq=want_all, mu=want_moments, s2=want_moments)
        fn = lead._lib.gpx_ensemble_sweep_dev if dev else lead._lib.gpx_ensemble_sweep
        lead._check(fn(_handles(engines), len(engines), acq_id(acq), _ptr(params), nparams, X, M, k, ptv, pti, _ptr(o['acq']), _ptr(o['mu']),
                       _ptr(o['s2'])))
        return dict(top_val=tv, top_idx=ti, **o)

    @staticmethod
    def ensemble_batch(engines, kind, param, nb):
        """nb greedy picks of the ensemble on its members' live sweep caches (gpx_ensemble_sweep_batch): the members frozen, each
        conditioned on a pick at its own posterior mean.  Returns dict(sel_val (nb,), sel_idx (nb,), sel_s2 (n, nb)); the members
        are left as they were."""
        lead = engines[0]
        params, nparams = _acq_params(param)
        n = max(int(nb), 0)
        out = dict(sel_val=np.empty(n), sel_idx=np.empty(n, dtype=np.int64), sel_s2=np.empty((len(engines), n)))
        lead._check(lead._lib.gpx_ensemble_sweep_batch(_handles(engines), len(engines), acq_id(kind), _ptr(params), nparams, int(nb),
                                                       _ptr(out['sel_val']), _ptr(out['sel_idx']), _ptr(out['sel_s2'])))
        return out

    @staticmethod
    def ensemble_predict(engines, Xc):
        """Per-member moments and gradients at the rows of Xc in ONE call (gpx_ensemble_predict):
        mu, s2 (n, M); dmu, ds2 (n, M, d)."""
        lead = engines[0]
        Xc = _f64(Xc).reshape(-1, lead.d)
        n, M, d = len(engines), len(Xc), lead.d
        mu, s2 = np.empty((n, M)), np.empty((n, M))
        dmu, ds2 = np.empty((n, M, d)), np.empty((n, M, d))
        lead._check(lead._lib.gpx_ensemble_predict(_handles(engines), n, _ptr(Xc), M, _ptr(mu), _ptr(s2), _ptr(dmu), _ptr(ds2)))
        return mu, s2, dmu, ds2

    @staticmethod
    def constrained_sweep(obj, cons, thr, acq, param, Xc, k=0, want_all=True, want_pof=False, d_acq=None, d_pof=None):
        """Constrained sweep (gpx_constrained_sweep[_dev]): EI / PI of the engine `obj` times the probability that every constraint engine
        of `cons` exceeds its threshold `thr[j]`; obj = None: the probability of feasibility alone (acq / param unread).  `Xc`: host
        array (M, d) or a DeviceGrid (then d_acq / d_pof: optional device pointers of (M,) vectors).  Returns dict(top_val, top_idx, acq,
        pof); the lead (obj, else cons[0]) raises the errors."""
        cons = list(cons)
        lead = obj if obj is not None else cons[0]
        thr = _f64(thr).reshape(-1)
        if len(thr) != len(cons):
            raise ValueError('one threshold per constraint')
        aid = acq_id(acq) if obj is not None else 0
        params, nparams = _acq_params(param)
        tv, ti, ptv, pti = _topk_out(k)
        dev, X, M, o = _candidates(Xc, lead.d, acq=want_all, pof=want_pof)
        fn = lead._lib.gpx_constrained_sweep_dev if dev else lead._lib.gpx_constrained_sweep
        outs = (_dptr(d_acq), _dptr(d_pof)) if dev else (_ptr(o['acq']), _ptr(o['pof']))
        lead._check(fn(obj._h if obj is not None else None, _handles(cons), len(cons), _ptr(thr), aid, _ptr(params), nparams, X, M, k, ptv, pti,
                       *outs))
        return dict(top_val=tv, top_idx=ti, **o)

    @staticmethod
    def constrained_batch(obj, cons, thr, acq, param, nb):
        """nb greedy picks of the constrained index on the members' live sweep caches (gpx_constrained_sweep_batch): EI / PI of the engine
        `obj` times every constraint engine's probability of exceeding `thr[j]`, target and thresholds frozen, every member conditioned
        on a pick at its own posterior mean; obj = None: the probability of feasibility alone (acq / param unread).  Returns
        dict(sel_val (nb,), sel_idx (nb,), sel_s2 (n, nb)), n = the members, the objective first; they are left as they were."""
        cons = list(cons)
        lead = obj if obj is not None else cons[0]
        thr = _f64(thr).reshape(-1)
        if len(thr) != len(cons):
            raise ValueError('one threshold per constraint')
        aid = acq_id(acq) if obj is not None else 0
        params, nparams = _acq_params(param)
        n = max(int(nb), 0)
        out = dict(sel_val=np.empty(n), sel_idx=np.empty(n, dtype=np.int64), sel_s2=np.empty((len(cons) + (obj is not None), n)))
        lead._check(lead._lib.gpx_constrained_sweep_batch(obj._h if obj is not None else None, _handles(cons), len(cons), _ptr(thr), aid,
                                                          _ptr(params), nparams, int(nb), _ptr(out['sel_val']), _ptr(out['sel_idx']),
                                                          _ptr(out['sel_s2'])))
        return out

    @staticmethod
    def _front_args(front, ref):
        front = np.ascontiguousarray(_f64(front if front is not None else np.empty((0, 2))).reshape(-1, 2))
        ref = np.ascontiguousarray(_f64(ref).reshape(-1))
        if len(ref) != 2:
            raise ValueError('the reference point has two coordinates')
        return front, ref

    @staticmethod
    def ehvi_sweep(f1, f2, front, ref, Xc, k=0, want_all=True, d_acq=None, d_mom=None):
        """Two-objective sweep (gpx_ehvi_sweep[_dev]): the expected hypervolume improvement of the engines `f1`, `f2` over the raw points
        `front` (np, 2) above `ref` (2), both host arrays.  `Xc`: host array (M, d) or a DeviceGrid (then d_acq / d_mom: optional device
        pointers of an (M,) and a (4, M) array: mu1, s2_1, mu2, s2_2).  Returns dict(top_val, top_idx, acq); f1 (the lead) raises the errors."""
        front, ref = Engine._front_args(front, ref)
        tv, ti, ptv, pti = _topk_out(k)
        dev, X, M, o = _candidates(Xc, f1.d, acq=want_all)
        args = (f1._h, f2._h, _ptr(front) if len(front) else None, len(front), _ptr(ref), X, M, k, ptv, pti)
        f1._check(f1._lib.gpx_ehvi_sweep_dev(*args, _dptr(d_acq), _dptr(d_mom)) if dev else f1._lib.gpx_ehvi_sweep(*args, _ptr(o['acq'])))
        return dict(top_val=tv, top_idx=ti, **o)

    @staticmethod
    def ehvi_batch(f1, f2, front, ref, nb):
        """nb greedy picks of the two-objective index on the engines' live sweep caches (gpx_ehvi_sweep_batch): both members and `ref`
        frozen, each member conditioned on a pick at its own posterior mean, and the pick's believed outcome (mu_1, mu_2) taken into the
        front -- on the device -- before the next round.  `front` (np, 2), `ref` (2): host arrays.  Returns dict(sel_val (nb,), sel_idx
        (nb,), sel_s2 (2, nb), sel_y (nb, 2) the believed outcomes, sel_nfront (nb,) the size of the front that scored each pick); the
        engines are left as they were, f1 (the lead) raises the errors."""
        front, ref = Engine._front_args(front, ref)
        n = max(int(nb), 0)
        out = dict(sel_val=np.empty(n), sel_idx=np.empty(n, dtype=np.int64), sel_s2=np.empty((2, n)), sel_y=np.empty((n, 2)),
                   sel_nfront=np.empty(n, dtype=np.int64))
        f1._check(f1._lib.gpx_ehvi_sweep_batch(f1._h, f2._h, _ptr(front) if len(front) else None, len(front), _ptr(ref), int(nb),
                                               *[_ptr(out[k]) for k in ('sel_val', 'sel_idx', 'sel_s2', 'sel_y', 'sel_nfront')]))
        return out

    def ehvi_fold(self, d_mom, M, front, ref, k=0, d_acq=None):
        """The fold and the top-k of a two-objective sweep alone (gpx_ehvi_fold_dev) on this engine's stream: `d_mom` the device pointer of
        a (4, M) array mu1, s2_1, mu2, s2_2 (e.g. of two `sweep_update` calls), `d_acq` an optional device pointer of (M,) values.
        Returns dict(top_val, top_idx)."""
        front, ref = Engine._front_args(front, ref)
        tv, ti, ptv, pti = _topk_out(k)
        self._check(self._lib.gpx_ehvi_fold_dev(self._h, _P(d_mom), int(M), _ptr(front) if len(front) else None, len(front), _ptr(ref), k, ptv, pti,
                                                _dptr(d_acq)))
        return dict(top_val=tv, top_idx=ti)

    def constrained_prune_report(self, vectors=True):
        """Diagnostic (gpx_constrained_prune_report in csrc/gpx_diag.h): what the last constrained sweep led by this engine decided about
        pruning.  dict(path, M, k, G, Gg, done, cap, nsurv, tau, gate, delta); with `vectors`, where the bound pass ran, also ub (M,), the
        objective's EI bound as the survivor pass read it, and idx, the survivors in compaction order (empty where it fell back)."""
        scal = np.full(11, np.nan)
        self._check(self._lib.gpx_constrained_prune_report(self._h, _ptr(scal), len(scal), None, None, 0))
        r = _report_head(scal)
        r.update(zip(('tau', 'gate', 'delta'), scal[8:].tolist()))
        return _report_vectors(r, vectors, lambda ub, idx, nidx: self._check(
            self._lib.gpx_constrained_prune_report(self._h, _ptr(scal), len(scal), ub, idx, nidx)))

    # -- Thompson --------------------------------------------------------------------------------
    def rff_gram(self, W, b):
        W = _f64(W)
        b = _f64(b)
        n = len(b)
        A = np.empty((n, n))
        v = np.empty(n)
        self._check(self._lib.gpx_rff_gram(self._h, _ptr(W), _ptr(b), n, _ptr(A), _ptr(v)))
        return A, v

    def rff_gram_batch(self, W, b):
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        A = np.empty((S, n, n))
        v = np.empty((S, n))
        self._check(self._lib.gpx_rff_gram_batch(self._h, _ptr(W), _ptr(b), S, n, _ptr(A), _ptr(v)))
        return A, v

    def rff_posterior(self, W, b, z, sc):
        """Weights theta (S, n) of S posterior draws: feature Grams and the n x n solves on the device."""
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        z = _f64(z).reshape(S, n)
        theta = np.empty((S, n))
        self._check(self._lib.gpx_rff_posterior(self._h, _ptr(W), _ptr(b), _ptr(z), S, n, float(sc), _ptr(theta)))
        return theta

    def rff_sweep(self, W, b, theta, bias, Xc, k=0, want_all=True):
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        theta = _f64(theta).reshape(S, n)
        Xc = _f64(Xc).reshape(-1, d)
        M = len(Xc)
        tv, ti, ptv, pti = _topk_out(k, S)
        out = np.empty((S, M)) if want_all else None
        self._check(self._lib.gpx_rff_sweep(self._h, _ptr(W), _ptr(b), _ptr(theta), S, n, d, bias, _ptr(Xc), M, k, ptv, pti, _ptr(out)))
        return dict(top_val=tv, top_idx=ti, vals=out)

    def rff_eval_grad(self, W, b, theta, bias, Xc):
        W = _f64(W)
        n, d = W.shape
        b = _f64(b)
        theta = _f64(theta)
        Xc = _f64(Xc).reshape(-1, d)
        M = len(Xc)
        f = np.empty(M)
        g = np.empty((M, d))
        self._check(self._lib.gpx_rff_grad(self._h, _ptr(W), _ptr(b), _ptr(theta), n, d, bias, _ptr(Xc), M,
                                           _ptr(f), _ptr(g)))
        return f, g

    def rff_sweep_dev(self, W, b, theta, bias, dXc_ptr, M, k):
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        theta = _f64(theta).reshape(S, n)
        tv = np.empty((S, k))
        ti = np.empty((S, k), dtype=np.int64)
        self._check(self._lib.gpx_rff_sweep_dev(self._h, _ptr(W), _ptr(b), _ptr(theta), S, n, d, bias,
                                                _P(dXc_ptr), M, k, _ptr(tv), _ptr(ti), None))
        return tv, ti

    # -- pathwise Thompson draws (the RFF draw as the prior, corrected exactly by the factorisation) -----
    def path_weights(self, W, b, w, eps, sc):
        """theta (S, n) = sc * w and v (S, N) = (K + sn2 I)^-1 ((y - bias) - Phi_s(X) theta_s - sqrt(sn2) eps_s) of S draws;
        w (S, n), eps (S, N) the caller's standard normals (eps None: zeros)."""
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        w = _f64(w).reshape(S, n)
        N = self.N
        if eps is not None:
            eps = _f64(eps).reshape(S, N)
        theta = np.empty((S, n))
        v = np.empty((S, N))
        self._check(self._lib.gpx_path_weights(self._h, _ptr(W), _ptr(b), _ptr(w), _ptr(eps), S, n, float(sc), _ptr(theta), _ptr(v)))
        return theta, v

    def path_sweep(self, W, b, theta, v, bias, Xc, k=0, want_all=True):
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        theta = _f64(theta).reshape(S, n)
        v = _f64(v).reshape(S, -1)
        Xc = _f64(Xc).reshape(-1, d)
        M = len(Xc)
        tv, ti, ptv, pti = _topk_out(k, S)
        out = np.empty((S, M)) if want_all else None
        self._check(self._lib.gpx_path_sweep(self._h, _ptr(W), _ptr(b), _ptr(theta), _ptr(v), v.shape[1], S, n, d, bias, _ptr(Xc), M, k, ptv, pti,
                                             _ptr(out)))
        return dict(top_val=tv, top_idx=ti, vals=out)

    def path_sweep_dev(self, W, b, theta, v, bias, dXc_ptr, M, k, d_vals=None):
        W = _f64(W)
        S, n, d = W.shape
        b = _f64(b).reshape(S, n)
        theta = _f64(theta).reshape(S, n)
        v = _f64(v).reshape(S, -1)
        tv, ti, ptv, pti = _topk_out(k, S)
        self._check(self._lib.gpx_path_sweep_dev(self._h, _ptr(W), _ptr(b), _ptr(theta), _ptr(v), v.shape[1], S, n, d, bias, _P(dXc_ptr), M, k, ptv,
                                                 pti, _dptr(d_vals)))
        return tv, ti

    def path_eval_grad(self, W, b, theta, v, bias, Xc):
        W = _f64(W)
        n, d = W.shape
        b = _f64(b)
        theta = _f64(theta)
        v = _f64(v).ravel()
        Xc = _f64(Xc).reshape(-1, d)
        M = len(Xc)
        f = np.empty(M)
        g = np.empty((M, d))
        self._check(self._lib.gpx_path_grad(self._h, _ptr(W), _ptr(b), _ptr(theta), _ptr(v), len(v), n, d, bias, _ptr(Xc), M,
                                            _ptr(f), _ptr(g)))
        return f, g

    # -- measurement -----------------------------------------------------------------------------
    def timers(self, reset=False):
        out = np.zeros(len(TIMER_NAMES))
        self._lib.gpx_timers(self._h, _ptr(out), len(out), 1 if reset else 0)
        return dict(zip(TIMER_NAMES, out.tolist()))

    PRUNE_PATHS = ('plain', 'gate declined', 'pruned', 'fell back')

    def prune_report(self, vectors=True):
        """Diagnostic (gpx_prune_report in csrc/gpx_diag.h): what the last sweep decided about pruning.  dict(path, M, k, G, Gg, done, cap,
        nsurv, S, delta, tau, gate_s2, thr_key, kept, bound_kernel = 'generic' / 'mfma' / 'mfma32' (None: no bound pass), guard = the matrix-pipe
        kernel's (d + 4)(R_x + R_z)^2 (NaN where the host chose the generic kernel)); with `vectors`, where the bound pass ran, also ub (M,) as the survivor pass read
        it and idx, the survivors in compaction order (empty where it fell back); after a sweep with option prune_keep = 1 also ub_kept
        and seed_idx, the bounds and the seed list before the scatter.  nR (block rows of the second bound's prefix, 0: it did not
        run) and nsurv2 (survivors of its cut); with `vectors`, nR > 0 and prune_keep = 1 also ub2, qR (aligned with idx) and idx2 (the
        second-level list).  E: the fp32 kernel's relative margin (NaN where it was not considered).  gate_hint: this sweep skipped its gate
        on the decision carried from the last one (csrc/prune_hint.h; then done = 0 and gate_s2 is NaN).  bound_fact: the fp32 kernel walked
        its factorised form (csrc/bound_f32.h; None where that kernel did not run) and bound_tpos, the first 16-row tile of its reordered
        weights without a positive one (None likewise)."""
        scal = np.full(22, np.nan)
        self._check(self._lib.gpx_prune_report(self._h, _ptr(scal), len(scal), None, None, 0, None, None, 0))
        r = _report_head(scal)
        r.update(zip(('S', 'delta', 'tau', 'gate_s2', 'thr_key', 'kept', 'bound_kernel', 'guard', 'nR', 'nsurv2', 'E', 'gate_hint', 'bound_fact',
                      'bound_tpos'), scal[8:].tolist()))
        r['bound_fact'] = None if np.isnan(r['bound_fact']) else r['bound_fact'] == 1.0
        r['bound_tpos'] = None if np.isnan(r['bound_tpos']) else int(r['bound_tpos'])
        r['gate_hint'] = r['gate_hint'] == 1.0
        r['bound_kernel'] = None if np.isnan(r['bound_kernel']) else ('generic', 'mfma', 'mfma32')[int(r['bound_kernel'])]
        for n in ('kept', 'nR', 'nsurv2'):
            r[n] = int(r[n])

        def fetch(ub, idx, nidx):
            kept = bool(r['kept'])
            r['ub_kept'] = np.empty(r['M']) if kept else None
            r['seed_idx'] = np.empty(r['G'], dtype=np.int64) if kept else None
            self._check(self._lib.gpx_prune_report(self._h, _ptr(scal), len(scal), ub, idx, nidx, _ptr(r['ub_kept']), _ptr(r['seed_idx']),
                                                   r['G'] if kept else 0))
            if r['nR'] > 0 and kept:
                r['ub2'] = np.empty(nidx)
                r['idx2'] = np.empty(r['nsurv2'], dtype=np.int64)
                r['qR'] = np.empty(nidx)
                self._check(self._lib.gpx_prune_rows(self._h, _ptr(r['qR']), _ptr(r['ub2']), _ptr(r['idx2']), r['nsurv2']))
        return _report_vectors(r, vectors, fetch)

    @staticmethod
    def ensemble_prune_report(engines, vectors=True):
        """Diagnostic (gpx_ensemble_prune_report in csrc/gpx_diag.h): what the last ensemble sweep led by engines[0] decided about pruning.
        dict(path, M, k, G, Gg, done, cap, nsurv, tau, gate, delta (n,), gate_hint: the gate was skipped on the carried decision); with `vectors`, where the bound pass ran, also ub (M,), the ensemble
        bound as the survivor pass read it, and idx, the survivors in compaction order (empty where it fell back).  bound_fact (n,): 1.0 where a
        member's dots came from the fp32 kernel's factorised walk, 0.0 from another kernel or form, NaN where the host chose the generic kernel."""
        lead, handles = engines[0], _handles(engines)
        scal = np.full(11 + 2 * len(engines), np.nan)
        lead._check(lead._lib.gpx_ensemble_prune_report(handles, len(engines), _ptr(scal), len(scal), None, None, 0))
        r = _report_head(scal)
        r.update(zip(('tau', 'gate'), scal[8:10].tolist()))
        r['delta'] = scal[10:10 + len(engines)].copy()
        r['gate_hint'] = scal[10 + len(engines)] == 1.0
        r['bound_fact'] = scal[11 + len(engines):11 + 2 * len(engines)].copy()
        return _report_vectors(r, vectors, lambda ub, idx, nidx: lead._check(
            lead._lib.gpx_ensemble_prune_report(handles, len(engines), _ptr(scal), len(scal), ub, idx, nidx)))

    def prune_dots(self):
        """Diagnostic (gpx_prune_dots): alpha2 . k(X, z_n) of the last pruned sweep's bound pass (option prune_keep = 1), before EI."""
        M = self.prune_report(vectors=False)['M']
        out = np.empty(M)
        self._check(self._lib.gpx_prune_dots(self._h, _ptr(out)))
        return out

    def chol_trace(self, nblocks, full_log=False):
        """Diagnostic (option chol_tg_trace = 1): the task-graph factorisation's own stamps of the last fit, microseconds
        from the first one: (diag (nblocks, 3) = wait / start / end per diagonal block, crit (nblocks, 8, 2) = the stamps of the
        workgroups that follow block row p -- slots 0, 1: S1 (waiting / right-hand sides loaded, .. / last rows stored), 2, 3: S2,
        4: U (waiting / earlier chunks in), 5: U (tile loaded / stored) -- see gpx_chol_trace in csrc/gpx_diag.h); None without a trace."""
        out = np.zeros(20 * nblocks + 8 * 1024 + 16 + (4 << 20 if full_log else 0), dtype=np.int64)
        n = self._lib.gpx_chol_trace(self._h, _ptr(out), out.size)
        if n < 20 * nblocks:
            return None
        self.last_chol_profile = out[20 * nblocks:20 * nblocks + 8192].reshape(1024, 8).copy()   # per workgroup (role index): see tg_trace.py
        self.last_chol_tasklog = None
        if full_log and n >= out.size:     # (option chol_tg_trace = 2) per workgroup 1024 records {task as 8 int16, start, end}
            self.last_chol_tasklog = out[20 * nblocks + 8192 + 16:].reshape(1024, 1024, 4).copy()
        out = out[:20 * nblocks]
        t0 = out[0]
        self.last_chol_trace_origin = int(t0)      # raw ticks of the first stamp (the task log's records are raw)
        diag = (out[:4 * nblocks].reshape(nblocks, 4)[:, :3] - t0) / 100.0
        crit = out[4 * nblocks:].reshape(nblocks, 8, 2).astype(np.float64)
        crit = np.where(crit > 0, (crit - t0) / 100.0, np.nan)
        return diag, crit

    def sync(self):
        self._check(self._lib.gpx_sync(self._h))
