"""The measurement behind profiles/con_batch_select.md: one process = one run at N = 8192 per member, d = 8, SE-ARD, M = 2^20 Sobol
candidates resident in HBM, an objective and J = 2 constraints (data and thresholds as tests/con_cases.py builds them).
   python scripts/con_batch_select_rate.py [reps] [ens-first]
The three cold cached sweeps (wall clock, each synchronised), then timer `batch` (slot 20) of the lead (the members' rank-1 passes of a batch
run inside it, not in slot 12) for gpx_constrained_sweep_batch (EI x feasibility) and, on THE SAME three handles, gpx_ensemble_sweep_batch (EI): after
one untimed nb = 8 call of each (allocation of the members' scratch), `reps` rounds of {constrained nb = 1, ensemble nb = 1, constrained
nb = 8, ensemble nb = 8}, the two forms alternating (`ens-first`: the ensemble's call in front of the constrained one in every pair: whichever
follows a short call starts on an idle device).  Prints one JSON line.  Run it under a `timeout`."""
import json, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from pybo_amd import _lib
from pybo_amd._lib import Engine, DeviceGrid
from helpers import synth_problem
import con_cases

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ens_first = len(sys.argv) > 2 and sys.argv[2] == 'ens-first'
N, d, M, J, NB = 8192, 8, 2 ** 20, 2, 8
X, y, ell = synth_problem(N, d, seed=0)
Cn = con_cases.constraint_data(X, 0, J)
thr = np.median(Cn, axis=0)
target = float(np.max(y[np.all(Cn >= thr, axis=1)]))
grid = DeviceGrid('sobol', [[0.0, 1.0]] * d, M, first=128)
out = dict(N=N, d=d, M=M, J=J, nb=NB, reps=reps, ens_first=ens_first, version=_lib.load().gpx_version())
engines, cold = [], []
for m, (sn2, rho, f, bias) in enumerate(con_cases.HYPERS[:1 + J]):
    e = Engine(0)
    e.fit(X, y if m == 0 else Cn[:, m - 1], 'se', ell * f, rho, sn2, bias)
    e.set_option('sweep_cache', 1)
    e.sync(); t0 = time.perf_counter()
    e.sweep_dev('ei' if m == 0 else 'pi', target if m == 0 else thr[m - 1], grid.ptr, M, 1)
    e.sync(); cold.append(1e3 * (time.perf_counter() - t0))
    e.set_option('sweep_cache', 0)
    engines.append(e)
obj, cons = engines[0], engines[1:]
forms = {'con': lambda nb: Engine.constrained_batch(obj, cons, thr, 'ei', target, nb),
         'ens': lambda nb: Engine.ensemble_batch(engines, 'ei', target, nb)}
if ens_first:
    forms = dict(reversed(list(forms.items())))
first = {k: f(NB) for k, f in forms.items()}            # allocation + first launches
times = {}
for rep in range(reps):
    for nb in (1, NB):
        for k, f in forms.items():
            for e in engines:
                e.timers(reset=True)
            t0 = time.perf_counter()
            got = f(nb)
            wall = 1e3 * (time.perf_counter() - t0)
            times.setdefault('%s_nb%d_ms' % (k, nb), []).append(engines[0].timers()['batch'])
            times.setdefault('%s_nb%d_wall_ms' % (k, nb), []).append(wall)
            assert np.array_equal(got['sel_idx'], first[k]['sel_idx'][:nb]) and np.array_equal(got['sel_val'], first[k]['sel_val'][:nb])
for k in forms:
    out['%s_per_extra_pick_ms' % k] = [(a - b) / (NB - 1) for a, b in zip(times['%s_nb%d_ms' % (k, NB)], times['%s_nb1_ms' % k])]
    out['%s_picks' % k] = first[k]['sel_idx'].tolist()
    out['%s_vals' % k] = first[k]['sel_val'].tolist()
out.update(cold_sweep_ms=cold, **times)
print(json.dumps(out))
