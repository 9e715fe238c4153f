"""The measurement behind profiles/mes_acq.md: what the acquisition line of a sweep costs for max-value entropy search (k_acq_mes,
S = 1, 16, 64 sampled maxima) against EI (k_acq) on the same handle, N = 8192, d = 8, SE-ARD, 2^20 candidates resident in HBM.
   python scripts/mes_rate.py [N [log2 M]]
Per acquisition, three repetitions each:
   cold    gpx_sweep_dev, k = 10, option prune = 0 (EI would otherwise skip candidates): timer slot 6 (acq_topk: the acquisition
           kernel of every chunk + one top-k), slot 4 (cross_gram) and slot 5 (sweep_trmm) of the same sweep, and the chunk count
   update  gpx_sweep_update on the cache that sweep seeded: slot 6 and the host's wall clock
   plugin  the warm step at the plug-in level: the second `index.topk(grid, 10)` of a policy index over a DeviceGrid (wall clock)
Prints one JSON line.  Run under a `timeout`."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

from pybo_amd import models, policies
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
cases = [('ei', 'ei', target)] + [('mes_S%d' % S, 'mes', target + 0.1 + 0.5 * rng.rand(S)) for S in (1, 16, 64)]
out = dict(N=N, d=d, M=M, k=K, reps=REPS)
e.sweep_dev('ei', target, grid.ptr, M, K)                   # first call: the inverse, the workspaces, the code objects
for name, kind, par in cases:
    rec = dict(cold_acq_ms=[], cold_xgram_ms=[], cold_trmm_ms=[], launches=[], update_acq_ms=[], update_wall_ms=[], plugin_wall_ms=[])
    for rep in range(REPS):
        e.set_option('sweep_cache', 1)
        e.timers(reset=True)
        e.sweep_dev(kind, par, grid.ptr, M, K)
        t = e.timers(reset=True)
        e.set_option('sweep_cache', 0)
        rec['cold_acq_ms'].append(round(t['acq_topk'], 4))
        rec['cold_xgram_ms'].append(round(t['cross_gram'], 3))
        rec['cold_trmm_ms'].append(round(t['sweep_trmm'], 3))
        rec['launches'].append(int(t['sweep_trmm_launches']))
        t0 = time.perf_counter()
        e.sweep_update(kind, par, k=K, want_all=False)
        rec['update_wall_ms'].append(round((time.perf_counter() - t0) * 1e3, 4))
        rec['update_acq_ms'].append(round(e.timers(reset=True)['acq_topk'], 4))
    out[name] = rec
e.set_option('sweep_cache', -1)
# the plug-in level: a policy index over the resident grid; its second topk is the warm re-score
for name, kind, par in cases:
    if kind == 'ei':
        index = policies.EI(gp, bounds, X)
    else:
        index = policies.MES(gp, bounds, X, nmax=len(par), ngrid=2000, rng=3)
    index.topk(grid, K)
    for rep in range(REPS):
        t0 = time.perf_counter()
        index.topk(grid, K)
        out[name]['plugin_wall_ms'].append(round((time.perf_counter() - t0) * 1e3, 4))
print(json.dumps(out))
