"""The measurement behind profiles/batch_fantasy.md: one process = one run at N = 8192, d = 8, SE-ARD, EI, M = 2^20 Sobol candidates.
   python scripts/batch_fantasy_rate.py time     timer `batch` (slot 20), five calls each, alternating in one loop: gpx_sweep_batch at
                                                 nb = 8 and nb = 1, gpx_sweep_batch_fantasy at nb = 8 for S = 1, 16, 64 x incumbent 0, 1
                                                 and at nb = 1 for S = 16
   python scripts/batch_fantasy_rate.py trace    one warmed call each of the believer and of S = 16, incumbent 1, nb = 8: to be run under a
                                                 kernel trace (k_batch_score against k_fant_score, k_batch_pick against k_fant_pick)
Prints one JSON line.  Run each under a `timeout`."""
import json, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from pybo_amd import _lib
from pybo_amd._lib import Engine, DeviceGrid
from helpers import synth_problem

mode = sys.argv[1]
N, d, M = 8192, 8, 2 ** 20
X, y, ell = synth_problem(N, d, seed=0)
e = Engine(0)
e.fit(X, y, 'se', ell, 1.0, 1e-3, 0.0)
grid = DeviceGrid('sobol', [[0.0, 1.0]] * d, M, first=128)
_, target = e.mean_at_obs()
e.set_option('sweep_cache', 1)
e.sweep_dev('ei', target, grid.ptr, M, 1)
e.set_option('sweep_cache', 0)
eps = np.random.RandomState(23).randn(64, 63)
out = dict(mode=mode, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + '/' + os.path.basename(_lib.LIB_PATH), version=_lib.load().gpx_version())


def timed(fn):
    e.timers(reset=True)
    r = fn()
    return e.timers()['batch'], r


bel = e.sweep_batch('ei', target, 8)                 # allocation + first launches
e.sweep_batch_fantasy('ei', target, 8, eps[:64], incumbent=1)
if mode == 'time':
    cols = {'believer_nb8': lambda: e.sweep_batch('ei', target, 8), 'believer_nb1': lambda: e.sweep_batch('ei', target, 1),
            'fantasy_S16_nb1': lambda: e.sweep_batch_fantasy('ei', target, 1, eps[:16], incumbent=1)}
    for S in (1, 16, 64):
        for inc in (0, 1):
            cols['fantasy_S%d_inc%d_nb8' % (S, inc)] = lambda S=S, inc=inc: e.sweep_batch_fantasy('ei', target, 8, eps[:S], incumbent=inc)
    ms = {k: [] for k in cols}
    picks = {}
    for rep in range(5):
        for k, fn in cols.items():
            t, r = timed(fn)
            ms[k].append(t)
            picks[k] = r['sel_idx'].tolist()
    zero = e.sweep_batch_fantasy('ei', target, 8, np.zeros((1, 7)), incumbent=0)
    out.update(ms=ms, picks=picks, zero_eps_is_believer=bool(all(np.array_equal(zero[k], bel[k]) for k in ('sel_val', 'sel_idx', 'sel_s2'))))
else:
    e.sweep_batch('ei', target, 8)
    e.sweep_batch_fantasy('ei', target, 8, eps[:16], incumbent=1)
    e.sync()
print(json.dumps(out))
