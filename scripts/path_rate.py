"""The measurement behind profiles/pathwise_thompson.md: one process = one shape.
   python scripts/path_rate.py d | e | ns [M]
       d, e: BASELINE configs D and E as bench.py defines them (make_workload, thompson_draw: N = 16384, d = 32, SE-ARD, 64 draws;
             N = 8192, d = 6, Matern-5/2, 8 draws; 100 features, M = 2^20 Sobol' candidates);
       ns:   N = 8192, d = 8, SE-ARD (bench.py's north-star model), S = 1 and S = 64.
   Per shape, three calls each after a warm-up call that grows the workspaces: gpx_path_sweep_dev and gpx_rff_sweep_dev with k = 1 (timer
   `rff`, slot 7: the kernels and the top-k; the host's wall clock around the call), gpx_path_weights and gpx_rff_posterior (wall clock),
   and timer `cross_gram` (slot 4) of one full EI sweep of the same candidates with pruning off.  For config D also the root mean square of
   f_s(X_i) - y_i over draws and observations, in units of sqrt(sn2), for both kinds of draw.
Prints one JSON line.  Run it under a `timeout`."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

import bench
from pybo_amd._lib import Engine
from test_gpu_prune import _dev

name = sys.argv[1]
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
w = bench.make_workload(name, M)
N, d, n = w['N'], w['d'], 100
e = Engine(0)
e.fit(w['X'], w['y'], w['kernel'], w['ell'], w['rho'], w['sn2'], w['bias'])
dXc = _dev(w['Xc'])
sc = np.sqrt(2.0 * w['rho'] / n)
out = dict(shape=name, N=N, d=d, M=M, n=n, kernel=w['kernel'])


def timed(call, reps=3):
    call()
    rows = []
    for rep in range(reps):
        e.timers(reset=True)
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        rows.append((round(e.timers()['rff'], 3), round(wall, 3)))
    return dict(rff_slot_ms=[r[0] for r in rows], wall_ms=[r[1] for r in rows])


for S in ((1, 64) if name == 'ns' else (8,) if name == 'e' else (64,)):
    draws = [bench.thompson_draw(w, s) for s in range(S)]
    W, b, z = (np.array([dr[i] for dr in draws]) for i in range(3))
    eps = np.random.RandomState(7).randn(S, N)
    res = dict(flop_update=2.0 * N * S * M)
    t0 = time.perf_counter()
    theta_rff = e.rff_posterior(W, b, z, sc)
    res['rff_posterior_wall_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
    e.path_weights(W, b, z, eps, sc)
    t0 = time.perf_counter()
    theta, v = e.path_weights(W, b, z, eps, sc)
    res['path_weights_wall_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
    res['rff_sweep_dev'] = timed(lambda: e.rff_sweep_dev(W, b, theta_rff, w['bias'], dXc.data_ptr(), M, 1))
    res['path_sweep_dev'] = timed(lambda: e.path_sweep_dev(W, b, theta, v, w['bias'], dXc.data_ptr(), M, 1))
    if name == 'd':
        sn = np.sqrt(w['sn2'])
        fp = e.path_sweep(W, b, theta, v, w['bias'], w['X'], k=0)['vals']
        fr = e.rff_sweep(W, b, theta_rff, w['bias'], w['X'], k=0)['vals']
        res['rms_at_data_over_sn'] = dict(pathwise=float(np.sqrt(np.mean((fp - w['y']) ** 2)) / sn), rff=float(np.sqrt(np.mean((fr - w['y']) ** 2)) / sn))
    out['S%d' % S] = res
e.set_option('prune', 0)
e.timers(reset=True)
e.sweep_dev('ei', float(np.max(w['y'])), dXc.data_ptr(), M, 1)
tm = e.timers()
out['ei_sweep'] = dict(cross_gram_ms=round(tm['cross_gram'], 3), sweep_trmm_ms=round(tm['sweep_trmm'], 3))
print(json.dumps(out))
