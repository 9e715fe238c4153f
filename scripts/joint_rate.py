"""The measurement behind profiles/joint_posterior.md: one process = one M at N = 8192, d = 8, SE-ARD, S = 64 draws.
   python scripts/joint_rate.py time M      per call of gpx_predict_cov and gpx_sample_joint (S = 64 and S = 1), five calls each after a
                                            warm-up call that grows the workspace: timer `joint` (slot 21: everything between the copies),
                                            timer `copies`, the host's wall clock around the call; a plain sweep of the same M points
                                            (timers `sweep_trmm`, `sweep_trmm_flop`, `cross_gram`) and of 65536 points for the rate beside
                                            the stored product's; and the numpy oracle's time for the same Sigma (the factor L is taken
                                            from the device, not timed).
   rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/joint_rate.py trace M
                                            the per-kernel split: one warm-up + three calls of each entry point and nothing else
   python scripts/joint_rate.py stats FILE_kernel_stats.csv
                                            that run's kernels grouped by stage, milliseconds per call (the warm-up included in the mean)
Prints one JSON line.  Run each under a `timeout`."""
import csv, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

N, d, S = 8192, 8, 64
mode = sys.argv[1]

# kernel-name fragments -> stage (the factorisation is launch_cholesky_small's kernels)
STAGES = (('k_cross_gram', 'cross_gram (K* and K**)'), ('k_scale_x', 'cross_gram (K* and K**)'), ('k_cov_trmm', 'stored product V = T K*'),
          ('k_cov_mu', 'mean'), ('k_cov_syrk', 'Sigma = K** - V^T V'), ('k_cov_form', 'factorisation'), ('k_potrf16', 'factorisation'),
          ('k_panel_solve16', 'factorisation'), ('k_row_update64', 'factorisation'), ('k_syrk_update', 'factorisation'),
          ('k_cov_draw', 'draws'))

if mode == 'stats':
    calls = {'cross_gram (K* and K**)': 8, 'stored product V = T K*': 8, 'mean': 8, 'Sigma = K** - V^T V': 8, 'factorisation': 4, 'draws': 4}
    tot = {}
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            for frag, stage in STAGES:
                if frag in row['Name']:
                    tot[stage] = tot.get(stage, 0.0) + float(row['TotalDurationNs']) * 1e-6
                    break
    print(json.dumps({'ms_per_call': {k: round(v / calls[k], 4) for k, v in tot.items()}}))
    sys.exit(0)

from pybo_amd._lib import Engine
from helpers import synth_problem

M = int(sys.argv[2])
X, y, ell = synth_problem(N, d, seed=0)
rho, sn2, bias = 1.0, 1e-3, 0.0
e = Engine(0)
e.fit(X, y, 'se', ell, rho, sn2, bias)
rng = np.random.RandomState(1)
Z, z = rng.rand(M, d), rng.randn(S, M)
jit = 1e-10 * rho
e.predict_cov(Z); e.sample_joint(Z, z, jitter=jit)          # first calls: the inverse, the workspace, the code objects
if mode == 'trace':
    for rep in range(3):
        e.predict_cov(Z); e.sample_joint(Z, z, jitter=jit)
    print(json.dumps(dict(mode=mode, M=M)))
    sys.exit(0)


def timed(call):
    e.timers(reset=True)
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = e.timers()
    return tm, wall


out = dict(mode=mode, N=N, d=d, M=M, S=S)
for name, call in (('predict_cov', lambda: e.predict_cov(Z)), ('sample_S64', lambda: e.sample_joint(Z, z, jitter=jit)),
                   ('sample_S1', lambda: e.sample_joint(Z, z[:1], jitter=jit))):
    rows = [timed(call) for rep in range(5)]
    out[name] = dict(joint_ms=[round(t['joint'], 4) for t, _ in rows], copies_ms=[round(t['copies'], 4) for t, _ in rows],
                     wall_ms=[round(w, 3) for _, w in rows])
for name, pts in (('sweep_same_M', Z), ('sweep_65536', rng.rand(65536, d))):
    e.predict(pts)
    rows = [timed(lambda: e.predict(pts))[0] for rep in range(3)]
    out[name] = dict(sweep_trmm_ms=[round(t['sweep_trmm'], 4) for t in rows], cross_gram_ms=[round(t['cross_gram'], 4) for t in rows],
                     tflops=[round(t['sweep_trmm_flop'] / t['sweep_trmm'] * 1e-9, 2) for t in rows])
out['stored_product_flop'] = float(N) * N * M            # the sweep's count: N^2 per point
# the oracle's Sigma on the host's BLAS threads, L given
import scipy.linalg as sla
from oracle import gp_ref
L = e.get_matrix('L')
ts = []
for rep in range(2):
    t0 = time.perf_counter()
    V = sla.solve_triangular(L, gp_ref.kernel(0, X, Z, ell, rho), lower=True)
    Sig = gp_ref.kernel(0, Z, Z, ell, rho) - V.T @ V
    ts.append(round((time.perf_counter() - t0) * 1e3, 1))
out['oracle_ms'] = ts
out['oracle_threads'] = int(os.environ.get('OMP_NUM_THREADS', '0'))
cov = e.predict_cov(Z)[1]
out['max_abs_diff_vs_oracle'] = float(np.abs(cov - Sig).max())
print(json.dumps(out))
