"""The measurement behind profiles/batch_select.md: one process = one run at N = 8192, d = 8, SE-ARD, EI, M = 2^20 Sobol candidates.
   python scripts/batch_select_rate.py batch     timer `batch` of gpx_sweep_batch, five calls each of nb = 8, 1, 2
   GPX_LIB_PATH=<parent commit's libgpx.so> python scripts/batch_select_rate.py rank1
                                                 timer `rank1` of one append_begin + append + sweep_update, five times
Prints one JSON line.  Run the two alternately in one job, each under a `timeout`."""
import json, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from pybo_amd import _lib
from pybo_amd._lib import Engine, DeviceGrid
from helpers import synth_problem

mode = sys.argv[1]
if mode == 'rank1':
    _lib.SYMBOLS.pop('gpx_sweep_batch', None)       # the parent commit's library has no such symbol
N, d, M = 8192, 8, 2 ** 20
X, y, ell = synth_problem(N, d, seed=0)
e = Engine(0)
e.fit(X, y, 'se', ell, 1.0, 1e-3, 0.0)
grid = DeviceGrid('sobol', [[0.0, 1.0]] * d, M, first=128)
_, target = e.mean_at_obs()
e.set_option('sweep_cache', 1)
e.sweep_dev('ei', target, grid.ptr, M, 1)
e.set_option('sweep_cache', 0)
out = dict(mode=mode, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + '/' + os.path.basename(_lib.LIB_PATH), version=_lib.load().gpx_version())
if mode == 'batch':
    e.sweep_batch('ei', target, 8)                  # allocation + first launches
    t8, t1, t2 = [], [], []
    for rep in range(5):
        e.timers(reset=True); e.sweep_batch('ei', target, 8); t8.append(e.timers()['batch'])
        e.timers(reset=True); e.sweep_batch('ei', target, 1); t1.append(e.timers()['batch'])
        e.timers(reset=True); e.sweep_batch('ei', target, 2); t2.append(e.timers()['batch'])
    out.update(batch_nb8_ms=t8, batch_nb1_ms=t1, batch_nb2_ms=t2)
else:
    rng = np.random.RandomState(1)
    r1, ap = [], []
    for rep in range(6):
        x = rng.rand(d)
        e.timers(reset=True)
        assert e.append_begin(x)
        assert e.append(x, float(np.sin(3 * x.sum())))
        e.sweep_update('ei', target, k=1, want_all=False)
        tm = e.timers()
        r1.append(tm['rank1']); ap.append(tm['append'])
    out.update(rank1_ms=r1[1:], append_ms=ap[1:])
print(json.dumps(out))
