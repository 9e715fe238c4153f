"""Two pruned EI sweeps at the headline shape (N = 8192, d = 8, 2^20 candidates) after one fit: the process a counters-only
rocprofv3 run wraps to read k_bound_mfma's counters (profiles/bound_exp_ab.md)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pybo_amd._lib import Engine

N, d, M = 8192, 8, 1 << 20
rng = np.random.RandomState(1)
X = rng.rand(N, d)
y = -((X - 0.5) ** 2).sum(1) + 1e-3 * rng.randn(N)
ell = 0.25 * np.ones(d)
rho, bias = float(np.var(y)), float(y.mean())
e = Engine(0)
e.set_option('prune', 1)
e.fit(X, y, 'se', ell, rho, 1e-4 * rho, bias)
Z = rng.rand(M, d)
for _ in range(2):
    e.sweep('ei', float(y.max()), Z, k=10, want_all=False)
print(e.timers())
