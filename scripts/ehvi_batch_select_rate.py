"""The measurement behind profiles/ehvi_batch_select.md: one process = one run at N = 8192 per member, d = 8, M = 2^20 Sobol candidates
resident in HBM, two objectives (data, kernels and hyper-parameters as tests/ehvi_cases.py builds them) and a staircase front of n points.
   python scripts/ehvi_batch_select_rate.py [n] [reps] [above|range]
`above` (default): the staircase lies above every observation, so a believed outcome is dominated unless the pick's means overshoot the
data, and the front keeps its n points (+ 1 or 2) through the batch -- every round's scoring pass folds n + 1 strips or so; `range`: it spans the observations' range (as the tests' do) and the
front follows the picks (sel_nfront is printed).  n + 7 <= 1024: the largest front an nb = 8 call takes has 1017 points.
The two cold cached sweeps (wall clock, each synchronised; they also leave the (4, M) moments in HBM), then timer `batch` (slot 20) of the
lead for gpx_ehvi_sweep_batch and, on THE SAME two handles in the same process, what the parent's code paths cost for the same work:
gpx_constrained_sweep_batch with the second objective as the one constraint (two correction passes and a table fold per extra pick) and
gpx_ehvi_fold_dev over the M moments at the same front (timer `acq_topk`, slot 6: the fold and its top-1).  After one untimed nb = 8 call of
each, `reps` rounds of {ehvi nb = 1, constrained nb = 1, ehvi nb = 8, constrained nb = 8, fold}.  Prints one JSON line.  Run it under a
`timeout`."""
import ctypes as C
import json, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from pybo_amd import _lib
from pybo_amd._lib import Engine, DeviceGrid
import ehvi_cases

nfront = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
place = sys.argv[3] if len(sys.argv) > 3 else 'above'
N, d, M, NB = 8192, 8, 2 ** 20, 8
p = ehvi_cases.build(N, d, 'se', 21, m=1)
X, Y = p['X'], p['Y']
lo, hi = (Y.max() + 0.3, Y.max() + 1.3) if place == 'above' else (Y.min(), Y.max())
if nfront:
    P, ref = ehvi_cases.raw_front(nfront, 3, lo=lo, hi=hi)
    ref = np.minimum(ref, Y.min(0) - 0.1 * (Y.max(0) - Y.min(0)))
else:
    P, ref = np.empty((0, 2)), Y.min(0) - 0.1 * (Y.max(0) - Y.min(0))
grid = DeviceGrid('sobol', [[0.0, 1.0]] * d, M, first=128)
lib = _lib.load()
hip = C.CDLL('libamdhip64.so')
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
dmom = C.c_void_p()
assert hip.hipMalloc(C.byref(dmom), 4 * M * 8) == 0
out = dict(N=N, d=d, M=M, nb=NB, n=nfront, place=place, reps=reps, version=lib.gpx_version())
engines, cold = [], []
for j, (sn2, rho, ell, bias) in enumerate(p['hypers']):
    e = Engine(0)
    e.fit(X, Y[:, j], p['kernels'][j], ell, rho, sn2, bias)
    e.set_option('sweep_cache', 1)
    e.sync(); t0 = time.perf_counter()
    e.sweep_dev('ei', float(ref[j]), grid.ptr, M, 1, d_mu=dmom.value + 2 * j * M * 8, d_s2=dmom.value + (2 * j + 1) * M * 8)
    e.sync(); cold.append(1e3 * (time.perf_counter() - t0))
    e.set_option('sweep_cache', 0)
    engines.append(e)
f1, f2 = engines
thr = float(np.median(Y[:, 1]))
forms = {'ehvi': lambda nb: Engine.ehvi_batch(f1, f2, P, ref, nb),
         'con': lambda nb: Engine.constrained_batch(f1, [f2], [thr], 'ei', float(ref[0]), nb)}
first = {k: f(NB) for k, f in forms.items()}            # allocation + first launches
f1.ehvi_fold(dmom.value, M, P, ref, k=1)
assert first['ehvi']['sel_nfront'][0] == nfront
times = {}
for rep in range(reps):
    for nb in (1, NB):
        for k, f in forms.items():
            for e in engines:
                e.timers(reset=True)
            t0 = time.perf_counter()
            got = f(nb)
            wall = 1e3 * (time.perf_counter() - t0)
            times.setdefault('%s_nb%d_ms' % (k, nb), []).append(f1.timers()['batch'])
            times.setdefault('%s_nb%d_wall_ms' % (k, nb), []).append(wall)
            assert np.array_equal(got['sel_idx'], first[k]['sel_idx'][:nb]) and np.array_equal(got['sel_val'], first[k]['sel_val'][:nb])
    f1.timers(reset=True)
    t0 = time.perf_counter()
    f1.ehvi_fold(dmom.value, M, P, ref, k=1)
    times.setdefault('fold_wall_ms', []).append(1e3 * (time.perf_counter() - t0))
    times.setdefault('fold_ms', []).append(f1.timers()['acq_topk'])
for k in forms:
    out['%s_per_extra_pick_ms' % k] = [(a - b) / (NB - 1) for a, b in zip(times['%s_nb%d_ms' % (k, NB)], times['%s_nb1_ms' % k])]
    out['%s_picks' % k] = first[k]['sel_idx'].tolist()
out.update(cold_sweep_ms=cold, nfront_per_round=first['ehvi']['sel_nfront'].tolist(), ehvi_vals=first['ehvi']['sel_val'].tolist(), **times)
print(json.dumps(out))
