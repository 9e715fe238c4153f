"""The measurement behind profiles/kg_acq.md: what a knowledge-gradient sweep (GPX_ACQ_KG, m = 16, 63, 127 support points) costs
against an EI sweep on the same handle, N = 8192, d = 8, SE-ARD, 2^20 candidates resident in HBM, and gpx_kg_grad at M = 10.
   python scripts/kg_rate.py [N [log2 M]]
Cold sweeps only (KG has no warm path), gpx_sweep_dev with every output (values, mu, s2: nothing is pruned, option prune = 0 besides),
k = 10, the acquisitions interleaved, three repetitions each.  Per sweep: timer slot 4 (cross_gram), 5 (sweep_trmm) and 6 (acq_topk:
for KG the support preparation, k_kg_cross and k_acq_kg of every chunk, and one top-k), and the host's wall clock.
   kg_mNN        a NEW support set per repetition (one coordinate moved): the preparation is paid
   kg_mNN_again  the same set again: the handle holds its preparation, slot 6 is products + values
so the preparation is the difference of the two.  The split between k_kg_cross and k_acq_kg is not visible to the timers: run this
script under `rocprofv3 --kernel-trace --stats` for it.  gpx_kg_grad: wall clock of a call with a prepared set, and with a new one.
Prints one JSON line.  Run under a `timeout`."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

from pybo_amd import models
from pybo_amd._lib import DeviceGrid
from helpers import synth_problem

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
M = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
d, K, REPS = 8, 10, 3
X, y, ell = synth_problem(N, d, seed=0)
bounds = np.array([[0.0, 1.0]] * d)
gp = models.make_gp(1e-3, 1.0, ell, 0.0)
gp.add_data(X, y)
e = gp._engine()
e.set_option('prune', 0)
grid = DeviceGrid('uniform', bounds, M, seed=1)
target = float(e.mean_at_obs()[1])
rng = np.random.RandomState(2)
supports = {m: rng.rand(m, d) for m in (16, 63, 127)}

import ctypes as C
hip = C.CDLL('libamdhip64.so')
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
bufs = []
for _ in range(3):                                          # acq_all, mu, s2 on the device: every output is asked for
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), M * 8) == 0
    bufs.append(p.value)


def sweep(kind, par):
    e.timers(reset=True)
    t0 = time.perf_counter()
    e.sweep_dev(kind, par, grid.ptr, M, K, d_acq=bufs[0], d_mu=bufs[1], d_s2=bufs[2])
    e.sync()
    wall = (time.perf_counter() - t0) * 1e3
    t = e.timers(reset=True)
    return dict(acq_ms=round(t['acq_topk'], 3), xgram_ms=round(t['cross_gram'], 3), trmm_ms=round(t['sweep_trmm'], 3),
                wall_ms=round(wall, 3), launches=int(t['sweep_trmm_launches']))


out = dict(N=N, d=d, M=M, k=K, reps=REPS)
sweep('ei', target)                                         # first call: the inverse, the workspaces, the code objects
sweep('kg', supports[16])
names = ['ei'] + ['kg_m%d' % m for m in supports] + ['kg_m%d_again' % m for m in supports]
for n in names:
    out[n] = []
for rep in range(REPS):
    out['ei'].append(sweep('ei', target))
    for m, A in supports.items():
        A = A.copy()
        A[0, 0] = 0.01 * (rep + 1)                          # a new set: prepared again
        out['kg_m%d' % m].append(sweep('kg', A))
        out['kg_m%d_again' % m].append(sweep('kg', A))
# gpx_kg_grad at M = 10: prepared set, then a new one
Zg = rng.rand(10, d)
A = supports[63]
e.kg_grad(A, Zg)
g = dict(prepared_wall_ms=[], new_set_wall_ms=[])
for rep in range(REPS):
    t0 = time.perf_counter()
    e.kg_grad(A, Zg)
    g['prepared_wall_ms'].append(round((time.perf_counter() - t0) * 1e3, 3))
    A2 = A.copy()
    A2[0, 0] = 0.02 * (rep + 1)
    t0 = time.perf_counter()
    e.kg_grad(A2, Zg)
    g['new_set_wall_ms'].append(round((time.perf_counter() - t0) * 1e3, 3))
    e.kg_grad(A, Zg)
out['kg_grad_M10_m63'] = g
print(json.dumps(out))
