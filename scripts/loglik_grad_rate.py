"""gpx_loglik_grad at N = 2048 and 8192 (d = 8, SE-ARD), one process, HIP events on the handle's stream (warm-up first, median
of 20): (a) the gradient on a fitted handle whose inverse exists, (b) fit + inverse + gradient end to end, (c) the only route
without it: d + 3 hyper-parameter vectors through gpx_loglik_batch (what a forward-difference gradient evaluates).  The
product's rate is N^3/3 multiply-adds (2 flop each) over (a), which also holds the reduction kernel, the evidence kernel and
the copy of d + 4 doubles.  Writes profiles/loglik_grad_rate.md when given --write."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
import numpy as np                      # noqa: E402
import torch                            # noqa: E402
from helpers import synth_problem       # noqa: E402
from pybo_amd import _lib               # noqa: E402

REPS = 20


def timed(stream, fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    stream = torch.cuda.Stream()
    eng = _lib.Engine(0, stream=stream.cuda_stream)
    rows = []
    for N, d in ((2048, 8), (8192, 8)):
        X, y, ell = synth_problem(N, d, seed=1)
        rho, sn2, bias = 1.2, 1.2e-2, 0.1
        eng.fit(X, y, 'se', ell, rho, sn2, bias)
        L, g = eng.loglik_grad()
        t_grad = timed(stream, eng.loglik_grad)
        t_all = timed(stream, lambda: (eng.fit(X, y, 'se', ell, rho, sn2, bias), eng.loglik_grad()), reps=REPS, warm=2)
        hyp = np.tile(np.concatenate([[sn2, rho], ell, [bias]]), (d + 3, 1))
        hyp[np.arange(d + 3), np.arange(d + 3)] *= 1.0 + 1e-6            # one perturbed component per vector
        t_fd = timed(stream, lambda: eng.loglik_batch(hyp), reps=REPS, warm=2)
        tf = 2.0 * N ** 3 / 3.0 / (t_grad * 1e-3) / 1e12
        rows.append((N, d, t_grad, tf, t_all, t_fd))
        print('N %5d d %d: gradient %.3f ms (%.1f TFLOP/s of N^3/3 FMAs), fit + inverse + gradient %.3f ms, %d vectors through '
              'gpx_loglik_batch %.3f ms;  L = %.10g' % (N, d, t_grad, tf, t_all, d + 3, t_fd, L), flush=True)
    eng.close()
    if '--write' in sys.argv:
        out = os.path.join(ROOT, 'profiles', 'loglik_grad_rate.md')
        with open(out, 'w') as f:
            f.write('# gpx_loglik_grad: measured times (scripts/loglik_grad_rate.py, one MI355X, SE-ARD, d = 8, median of %d)\n\n' % REPS)
            f.write('| N | gradient, inverse present (ms) | product rate (TFLOP/s, 2 N^3/3 flop) | fit + inverse + gradient (ms) | '
                    'd + 3 = 11 vectors through gpx_loglik_batch (ms) |\n|---|---|---|---|---|\n')
            for N, d, a, tf, b, c in rows:
                f.write('| %d | %.3f | %.1f | %.3f | %.3f |\n' % (N, a, tf, b, c))
        print('wrote', out)


if __name__ == '__main__':
    main()
