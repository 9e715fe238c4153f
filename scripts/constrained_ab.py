"""A/B of the constrained sweep on the headline shape: N = 8192, d = 8, SE-ARD, 2^20 uniform candidates resident
in HBM, J = 2 constraints, k = 10.  Data, constraint observations, thresholds and hyper-parameters as tests/con_cases.py builds them
at that size.  Three arms, alternated, `--repeats` timed rounds after `--warmup` untimed ones:

  (a) the composition a caller had before gpx_constrained_sweep: 1 + J gpx_sweep_dev calls with d_acq_all into torch tensors, a torch
      product (each factor clamped at 1, in constraint order) and torch.topk
  (b) gpx_constrained_sweep_dev with the objective's option prune = 0
  (c) the same with prune = -1 (the automatic rule)

Times are host clock around calls that end in a synchronisation.  Per arm the stage timers of every handle are recorded too (slots 4
cross_gram, 5 sweep_trmm, 6 acq_topk, 19 sweep_bound, and the sweep_trmm launches), and the share of (1 + J) N^2 M that was evaluated.
Writes a markdown report (--out) and prints one JSON line.

    python scripts/constrained_ab.py --out profiles/constrained_sweep.md
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

import con_cases        # noqa: E402
from pybo_amd._lib import Engine, DeviceGrid      # noqa: E402

SLOTS = ('cross_gram', 'sweep_trmm', 'acq_topk', 'sweep_bound', 'sweep_trmm_launches', 'sweep_trmm_flop')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=8192)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--M', type=int, default=1 << 20)
    ap.add_argument('--J', type=int, default=2)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--seed', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'constrained_sweep.md'))
    a = ap.parse_args()
    N, d, M, J, k = a.N, a.d, a.M, a.J, a.k

    p = con_cases.build(N, d, 'se', a.seed, J, m=1)
    engines = []
    for i, (sn2, rho, ell, bias) in enumerate(p['hypers']):
        e = Engine(0)
        e.fit(p['X'], p['y'] if i == 0 else p['C'][:, i - 1], 'se', ell, rho, sn2, bias)
        engines.append(e)
    obj, cons = engines[0], engines[1:]
    grid = DeviceGrid('uniform', [[0.0, 1.0]] * d, M, seed=a.seed + 100)
    thr, target = p['thr'], p['target']
    bufs = [torch.empty(M, dtype=torch.float64, device='cuda') for _ in range(1 + J)]
    one = torch.ones((), dtype=torch.float64, device='cuda')

    def arm_a():
        obj.set_option('prune', 0)
        obj.sweep_dev('ei', target, grid.ptr, M, 0, d_acq=bufs[0].data_ptr())
        for j, c in enumerate(cons):
            c.sweep_dev('pi', thr[j], grid.ptr, M, 0, d_acq=bufs[1 + j].data_ptr())
        v = bufs[0]
        for j in range(J):
            v = v * torch.minimum(bufs[1 + j], one)
        tv, ti = torch.topk(v, k)
        return tv.cpu().numpy(), ti.cpu().numpy()

    def arm(prune):
        def run():
            obj.set_option('prune', prune)
            r = Engine.constrained_sweep(obj, cons, thr, 'ei', target, grid, k=k)
            return r['top_val'], r['top_idx']
        return run

    arms = [('a', 'composition: 1 + J gpx_sweep_dev, torch product, torch.topk', arm_a),
            ('b', 'gpx_constrained_sweep_dev, prune = 0', arm(0)),
            ('c', 'gpx_constrained_sweep_dev, prune = -1', arm(-1))]
    times = {n: [] for n, _, _ in arms}
    stage = {n: None for n, _, _ in arms}
    result, report = {}, {}
    for rnd in range(a.warmup + a.repeats):
        for name, _, fn in arms:
            for e in engines:
                e.timers(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3
            tm = [e.timers(reset=True) for e in engines]
            if rnd >= a.warmup:
                times[name].append(dt)
                stage[name] = [{s: t[s] for s in SLOTS} for t in tm]
            result[name] = out
            if name != 'a':
                report[name] = obj.constrained_prune_report(vectors=False)
            print('round %d arm %s: %.2f ms' % (rnd, name, dt), flush=True)

    full = (1 + J) * float(N) * float(N) * float(M)
    share = {n: sum(s['sweep_trmm_flop'] for s in stage[n]) / full for n in stage}
    same = {'a_b': bool(np.array_equal(result['a'][0], result['b'][0]) and np.array_equal(result['a'][1], result['b'][1])),
            'b_c': bool(np.array_equal(result['b'][0], result['c'][0]) and np.array_equal(result['b'][1], result['c'][1]))}
    stats = {n: dict(mean=float(np.mean(t)), min=float(np.min(t)), max=float(np.max(t)), n=len(t)) for n, t in times.items()}
    lines = ['# Constrained sweep: composition against gpx_constrained_sweep_dev, plain and pruned', '',
             'Written by `scripts/constrained_ab.py`.  N = %d, d = %d, SE-ARD, M = %d uniform candidates in a `DeviceGrid`, J = %d, k = %d;' % (N, d, M, J, k),
             'data, constraints, thresholds and hyper-parameters as `tests/con_cases.py` builds them at this size (seed %d).  %d warm-up round(s),' % (a.seed, a.warmup),
             '%d timed rounds, the arms alternated; host clock around calls that end in a synchronisation.' % a.repeats, '',
             '| arm | what | mean ms | min | max | share of (1 + J) N^2 M evaluated |', '|---|---|---|---|---|---|']
    for name, what, _ in arms:
        s = stats[name]
        lines.append('| (%s) | %s | %.2f | %.2f | %.2f | %.5f |' % (name, what, s['mean'], s['min'], s['max'], share[name]))
    lines += ['', 'Top-k (value and index) `array_equal`: (a) against (b) **%s**, (b) against (c) **%s**.' % (same['a_b'], same['b_c']), '']
    for n in ('b', 'c'):
        r = report[n]
        lines.append('Report of (%s): path `%s`, gate %s (mean s2 of the objective over Gg = %d; rho / 64 = %.4g), G = %d, nsurv = %d of cap %d, tau = %.4g.'
                     % (n, r['path'], '%.4g' % r['gate'], r['Gg'], p['hypers'][0][1] / 64.0, r['G'], r['nsurv'], r['cap'], r['tau']))
    lines += ['', 'Stage timers of the last timed round, ms (objective, then the constraints in order):', "(HIP events on each handle's own stream.  In (a) the three k = 0 sweeps return without a host synchronisation and overlap on the device, and in (b) a constraint's events also span the time its stream waits for the chip: the per-handle times of (a) and (b) do not add up to the wall clock.)", '',
              '| arm | handle | cross_gram [4] | sweep_trmm [5] | acq_topk [6] | sweep_bound [19] | sweep_trmm launches |', '|---|---|---|---|---|---|---|']
    for name, _, _ in arms:
        for i, s in enumerate(stage[name]):
            lines.append('| (%s) | %s | %.2f | %.2f | %.2f | %.2f | %d |' % (name, 'objective' if i == 0 else 'constraint %d' % i, s['cross_gram'],
                                                                             s['sweep_trmm'], s['acq_topk'], s['sweep_bound'], int(s['sweep_trmm_launches'])))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)
    print(text)
    print(json.dumps(dict(shape=dict(N=N, d=d, M=M, J=J, k=k), ms=stats, share=share, topk_equal=same,
                          report={n: {q: (None if isinstance(v, float) and np.isnan(v) else v) for q, v in r.items()} for n, r in report.items()})))
    grid.close()


if __name__ == '__main__':
    main()
