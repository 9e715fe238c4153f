"""A/B of the two-objective sweep on the headline shape: N = 8192, d = 8, 2^20 uniform candidates resident in
HBM, k = 10, fronts of n = 0, 16, 256, 1024 points (tests/ehvi_cases.py: raw_front, scaled to the observations' range).  Data and
hyper-parameters as tests/ehvi_cases.py builds them at that size (objective 1 SE-ARD, objective 2 Matern-5/2).  Per front size:

  (call)  gpx_ehvi_sweep_dev for the top-k, the moments kept in a torch tensor
  (fold)  gpx_ehvi_fold_dev alone on those moments (k = 0), between torch events on the lead's stream, and the library's own stage timer
          of the kernel (slot 6); ms per strip = kernel time / (n + 1)
  (comp)  the composition the call replaces: two gpx_sweep_dev(GPX_ACQ_MEAN) with moments into torch tensors, the D2H copy of the 4 M
          moments, and the numpy closed form (pybo_amd.pareto.ehvi_from_moments) + argpartition; the numpy part is timed ONCE per
          front size (it takes minutes at n = 1024), the device part over the rounds

`--repeats` timed rounds after `--warmup` untimed ones, host clock around calls that end in a synchronisation.  Also recorded: the
largest |kernel - numpy| / S over every 16th candidate per front size (S: the magnitude sum of tests/ehvi_ref.py), which the kernel test
bounds by 1e-9.  Writes a markdown report (--out) and prints one JSON line.

    python scripts/ehvi_ab.py --out profiles/ehvi_sweep.md
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np      # noqa: E402
import torch            # noqa: E402

import ehvi_cases       # noqa: E402
import ehvi_ref         # noqa: E402
from pybo_amd import pareto      # noqa: E402
from pybo_amd._lib import Engine, DeviceGrid      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=8192)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--M', type=int, default=1 << 20)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--fronts', default='0,16,256,1024')
    ap.add_argument('--seed', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ehvi_sweep.md'))
    a = ap.parse_args()
    N, d, M, k = a.N, a.d, a.M, a.k
    fronts = [int(x) for x in a.fronts.split(',')]

    p = ehvi_cases.build(N, d, 'se', a.seed, m=1)
    stream = torch.cuda.Stream()
    engines = []
    for j, (sn2, rho, ell, bias) in enumerate(p['hypers']):
        e = Engine(0, stream=stream.cuda_stream if j == 0 else None)
        e.fit(p['X'], p['Y'][:, j], p['kernels'][j], ell, rho, sn2, bias)
        engines.append(e)
    f1, f2 = engines
    grid = DeviceGrid('uniform', [[0.0, 1.0]] * d, M, seed=a.seed + 100)
    lo, hi = float(p['Y'].min()), float(p['Y'].max())
    mom = torch.empty((4, M), dtype=torch.float64, device='cuda')
    comp = torch.empty((4, M), dtype=torch.float64, device='cuda')
    vals = torch.empty(M, dtype=torch.float64, device='cuda')
    rows = []
    for n in fronts:
        P, ref = ehvi_cases.raw_front(n, seed=a.seed + n, lo=lo, hi=hi) if n else (np.empty((0, 2)), np.array([lo - 0.5, lo - 0.5]))
        sa, sb = pareto.strips(P, ref)
        assert len(sb) - 1 == n
        t_call, t_fold, t_kern, t_dev = [], [], [], []
        for rnd in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = Engine.ehvi_sweep(f1, f2, P, ref, grid, k=k, d_mom=mom.data_ptr())
            dt_call = (time.perf_counter() - t0) * 1e3
            f1.timers(reset=True)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            f1.ehvi_fold(mom.data_ptr(), M, P, ref, k=0, d_acq=vals.data_ptr())
            ev1.record(stream)
            ev1.synchronize()
            dt_fold, dt_kern = ev0.elapsed_time(ev1), f1.timers(reset=True)['acq_topk']
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j, f in enumerate(engines):
                f.sweep_dev('mean', None, grid.ptr, M, 0, d_mu=comp[2 * j].data_ptr(), d_s2=comp[2 * j + 1].data_ptr())
            for f in engines:
                f.sync()
            hmom = comp.cpu().numpy()
            dt_dev = (time.perf_counter() - t0) * 1e3
            if rnd >= a.warmup:
                t_call.append(dt_call), t_fold.append(dt_fold), t_kern.append(dt_kern), t_dev.append(dt_dev)
            print('n %d round %d: call %.2f ms, fold %.3f ms (kernel %.3f), two sweeps + D2H %.2f ms' % (n, rnd, dt_call, dt_fold, dt_kern, dt_dev), flush=True)
        same_mom = bool(np.array_equal(hmom, mom.cpu().numpy()))
        t0 = time.perf_counter()
        want = pareto.ehvi_from_moments(*hmom, sa, sb)
        top = np.argpartition(-want, k)[:k]
        top = top[np.lexsort((top, -want[top]))]
        dt_numpy = (time.perf_counter() - t0) * 1e3
        got = vals.cpu().numpy()
        sub = np.arange(0, M, max(1, M // 65536))          # (every 16th candidate at 2^20: S costs 2 (n + 1) EI evaluations per candidate)
        S = np.concatenate([ehvi_ref.magnitude(*hmom[:, sub[q:q + 2048]], sa, sb) for q in range(0, len(sub), 2048)])
        ok = S > 1e-290
        worst = float(np.max(np.abs(got[sub] - want[sub])[ok] / S[ok])) if ok.any() else 0.0
        rows.append(dict(n=n, call=float(np.mean(t_call)), fold=float(np.mean(t_fold)), kernel=float(np.mean(t_kern)), per_strip=float(np.mean(t_kern)) / (n + 1),
                         dev=float(np.mean(t_dev)), numpy=dt_numpy, comp=float(np.mean(t_dev)) + dt_numpy, same_moments=same_mom,
                         same_topk=bool(np.array_equal(top, r['top_idx'])), worst_err_over_S=worst, best=float(r['top_val'][0])))
        print(json.dumps(rows[-1]), flush=True)

    lines = ['# Two-objective sweep: gpx_ehvi_sweep_dev, its fold alone, and the composition it replaces', '',
             'Written by `scripts/ehvi_ab.py`.  N = %d, d = %d, objective 1 SE-ARD, objective 2 Matern-5/2, M = %d uniform candidates in a `DeviceGrid`, k = %d;' % (N, d, M, k),
             'data and hyper-parameters as `tests/ehvi_cases.py` builds them at this size (seed %d); fronts: `ehvi_cases.raw_front` over the range of the observations.' % a.seed,
             '%d warm-up round(s), %d timed rounds (means), host clock around calls that end in a synchronisation; the fold between torch events on the' % (a.warmup, a.repeats),
             "lead's stream (strip upload + kernel), `kernel` = the library's stage timer [6] of the same call; the numpy closed form timed once.", '',
             '| front n | call ms | fold alone ms | kernel ms | kernel ms per strip | two MEAN sweeps + D2H ms | numpy closed form + top-k ms | composition ms | call / composition |',
             '|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append('| %d | %.1f | %.3f | %.3f | %.5f | %.1f | %.0f | %.0f | %.3f |' % (r['n'], r['call'], r['fold'], r['kernel'], r['per_strip'], r['dev'], r['numpy'], r['comp'],
                                                                                     r['call'] / r['comp']))
    lines += ['', '| front n | moments of the call `array_equal` the two sweeps\' | top-k indices equal numpy\'s | largest abs(kernel - numpy) / S | best value |', '|---|---|---|---|---|']
    for r in rows:
        lines.append('| %d | %s | %s | %.3g | %.6g |' % (r['n'], r['same_moments'], r['same_topk'], r['worst_err_over_S'], r['best']))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)
    print(text)
    print(json.dumps(dict(shape=dict(N=N, d=d, M=M, k=k), rows=rows)))
    grid.close()


if __name__ == '__main__':
    main()
