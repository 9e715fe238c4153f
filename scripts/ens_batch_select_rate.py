"""The measurement behind profiles/ens_batch_select.md: one process = one run at N = 8192, d = 8, SE-ARD, EI, M = 2^20 Sobol
candidates resident in HBM, 10 ensemble members.
   python scripts/ens_batch_select_rate.py device   the n cold cached sweeps (wall clock, each synchronised), then timer `batch` of
                                                    gpx_ensemble_sweep_batch on the lead: three calls each of nb = 1, 2, 8, 16
                                                    after one untimed call (allocation of the members' scratch)
   python scripts/ens_batch_select_rate.py host     the generic host path (pybo_amd.batch._host_batch) on a models.MCMC of the same
                                                    size, nb = 2, wall clock -- also runs from a checkout of the commit before
                                                    gpx_ensemble_sweep_batch, where it is the only path
Prints one JSON line.  Run each under a `timeout`."""
import json, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from pybo_amd import _lib
from pybo_amd._lib import Engine, DeviceGrid
from helpers import synth_problem

mode = sys.argv[1]
N, d, M, NMEM = 8192, 8, 2 ** 20, 10
X, y, ell = synth_problem(N, d, seed=0)
grid = DeviceGrid('sobol', [[0.0, 1.0]] * d, M, first=128)
out = dict(mode=mode, N=N, d=d, M=M, members=NMEM, version=_lib.load().gpx_version())
if mode == 'device':
    engines = []
    for m in range(NMEM):       # members spread around one model, as tests/ens_batch_ref.member_hypers spreads them
        e = Engine(0)
        e.fit(X, y, 'se', ell * (1.0 + 0.03 * (m - (NMEM - 1) / 2.0)), 1.0 + 0.05 * m, 1e-3 * (1 + m), 0.01 * m)
        engines.append(e)
    target = float(np.mean([e.mean_at_obs()[0] for e in engines], axis=0).max())
    cold = []
    for e in engines:
        e.set_option('sweep_cache', 1)
        e.sync(); t0 = time.perf_counter()
        e.sweep_dev('ei', target, grid.ptr, M, 1)
        e.sync(); cold.append(1e3 * (time.perf_counter() - t0))
        e.set_option('sweep_cache', 0)
    lead = engines[0]
    first = Engine.ensemble_batch(engines, 'ei', target, 16)            # allocation + first launches
    times = {}
    for rep in range(3):
        for nb in (1, 2, 8, 16):
            lead.timers(reset=True)
            t0 = time.perf_counter()
            got = Engine.ensemble_batch(engines, 'ei', target, nb)
            wall = 1e3 * (time.perf_counter() - t0)
            times.setdefault('nb%d_ms' % nb, []).append(lead.timers()['batch'])
            times.setdefault('nb%d_wall_ms' % nb, []).append(wall)
            assert np.array_equal(got['sel_idx'], first['sel_idx'][:nb])
    out.update(cold_sweep_ms=cold, picks=first['sel_idx'].tolist(), distinct=len(set(first['sel_idx'].tolist())), **times)
else:
    from pybo_amd import models, batch
    gp = models.make_gp(1e-3, 1.0, ell, 0.0)
    gp.params['like.sn2'].set_prior('lognormal', np.log(1e-3), 1.0)
    gp.params['kern.rho'].set_prior('lognormal', 0.0, 1.0)
    gp.params['kern.ell'].set_prior('uniform', [0.02] * d, [3.0] * d)
    gp.params['mean.bias'].set_prior('normal', 0.0, 4.0)
    gp.add_data(X, y)
    t0 = time.perf_counter()
    mc = models.MCMC(gp, n=NMEM, burn=2, rng=0)
    out['construct_s'] = time.perf_counter() - t0
    target = float(mc.predict_mean(X).max())
    Z = np.asarray(grid)
    t0 = time.perf_counter()
    vals, idx = batch._host_batch(mc, 'ei', target, Z, 2)
    out.update(host_nb2_s=time.perf_counter() - t0, picks=idx.tolist())
print(json.dumps(out))
