"""k_bound_mfma with the table-driven exponential (csrc/bound_exp.h), the norms through the accumulator and the one-instruction
limits.

  probe     the construction of tests/test_gpu_devmath.py: one observation at x = 0, d = 1, ell = 1, rho = 1, sn2 = 3, y = 4, bias = 0,
            so the weight rho alpha~ is exactly 1 and the centre is 0: the kernel's exponent is exactly -fl(z^2) / 2 and
            Engine.prune_dots() IS bound_exp at that argument.  Held array_equal to the host checker's output for the same
            arguments (tests/c/bound_exp_check.cpp: the header the kernel includes), 0 and the tail below -746 included, and within
            the host test's 1.05 ulp of mpmath; a NaN candidate gives NaN;
  layouts   d in {1, 2, 3, 4, 7, 8, 11, 12, 15, 16, 18} (d mod 4 in {0, 3}: norms through the accumulator, one MFMA fewer; {1, 2}: the
            layout as it was), N in {128, 130}: every invariant of tests/test_gpu_prune_bound.py (check_sweep, pruned top-k array_equal
            plain) with either kernel forced, the two kernels' dots within u ((d + 4)(R_x + R_z)^2 + 3) rho S
            (tests/test_gpu_prune_bound_mfma.py: _agree), NaN in the same places;
  walk      N = 2049, d = 8: 129 row tiles, uneven over the four waves;
  edge      M = 3 * 4096 + 1: the last workgroup owns one live column; that candidate sits on an observation; a NaN coordinate
            elsewhere gives NaN under both kernels, an infinite one (forced past the guard) NaN and nothing finite."""
import subprocess

import mpmath as mp
import numpy as np
import pytest

from test_bound_exp_host import ULP_BOUND, build_checker
from test_gpu_prune_bound import _engine, _problem, check_sweep
from test_gpu_prune_bound_mfma import _agree, _run

pytestmark = pytest.mark.gpu

G = 4096
M = 3 * G + 1
LN2 = 0.6931471805599453


def _host_values(tmp_path, x):
    exe = build_checker(tmp_path)
    fin, fout = tmp_path / 'args.bin', tmp_path / 'vals.bin'
    np.ascontiguousarray(x, dtype=np.float64).tofile(str(fin))
    subprocess.check_call([exe, str(fin), str(fout)])
    got = np.fromfile(str(fout), dtype=np.float64)
    assert got.shape == x.shape
    return got


def test_the_kernel_s_exponential_is_the_host_checker_s_bit_for_bit(tmp_path):
    from pybo_amd._lib import Engine
    rng = np.random.RandomState(11)
    k = np.arange(-4 * 128, 1)
    want_x = np.concatenate([-60.0 * rng.rand(5500), -746.0 * rng.rand(4500), -1e-3 * rng.rand(400),
                             k * LN2 / 128, (k - 0.5) * LN2 / 128, [0.0, -745.2, -746.0, -748.0, -800.0, -5e9]])
    z = np.sqrt(-2.0 * want_x)
    z = np.concatenate([z, np.nextafter(z[:M - 1 - len(z)], np.inf)])
    assert len(z) == M - 1
    z = np.concatenate([z, [np.nan]])
    x = -0.5 * (z * z)                               # the kernel's own argument: fl(z^2) halved, exactly
    e = Engine(0)
    for name, v in (('prune_keep', 1), ('prune', 1), ('prune_bound', 1)):
        e.set_option(name, v)
    e.fit(np.zeros((1, 1)), np.array([4.0]), 'se', [1.0], 1.0, 3.0, 0.0)
    assert e.get_matrix('T')[0, 0] == 0.5 and e.get_vectors()[0][0] == 2.0
    e.sweep('ei', 0.5, z[:, None], k=10, want_all=False)
    r = e.prune_report(vectors=False)
    assert r['path'] in ('pruned', 'fell back') and r['bound_kernel'] == 'mfma', r
    dots = e.prune_dots()
    e.close()
    assert np.isnan(dots[-1]) and not np.isnan(dots[:-1]).any()
    host = _host_values(tmp_path, x[:-1])
    assert np.array_equal(dots[:-1], host), np.flatnonzero(dots[:-1] != host)[:8]
    assert dots[z == 0.0][0] == 1.0 and np.all(dots[:-1][x[:-1] <= -746.0] == 0.0)
    mp.mp.dps = 50
    worst = 0.0
    for xi, got in zip(x[:-1], dots[:-1]):
        want = mp.exp(mp.mpf(float(xi)))
        if want >= mp.mpf(2) ** -1022:
            ulp = mp.mpf(2) ** (mp.floor(mp.log(want, 2)) - 52)
            worst = max(worst, float(abs(mp.mpf(float(got)) - want) / ulp))
    print('device bound_exp: max error %.4f ulp over %d arguments' % (worst, M - 1))
    assert worst <= ULP_BOUND


def _both_kernels(w, Z, label):
    e = _engine(w)
    r1 = _run(e, w, Z, 10, 1, label=label)
    assert r1['bound_kernel'] == 'mfma' and r1['path'] in ('pruned', 'fell back'), label
    r0 = _run(e, w, Z, 10, 0, label=label)
    assert r0['bound_kernel'] == 'generic' and r0['path'] in ('pruned', 'fell back'), label
    _agree(r0, r1, w, label)
    e.close()
    return r0, r1


@pytest.mark.parametrize('N', [128, 130])
@pytest.mark.parametrize('d', [1, 2, 3, 4, 7, 8, 11, 12, 15, 16, 18])
def test_every_layout_keeps_the_invariants_and_agrees_with_the_generic_kernel(d, N):
    w = _problem(N, d, M, 'se', seed=13 * N + d)
    _both_kernels(w, w['Xc'], 'N=%d d=%d' % (N, d))


def test_a_walk_that_is_uneven_over_the_waves():
    w = _problem(2049, 8, M, 'se', seed=23)
    _both_kernels(w, w['Xc'], 'N=2049 d=8')


def test_the_single_live_column_of_the_last_workgroup_and_the_candidates_without_a_finite_norm():
    assert M % 128 == 1
    w = _problem(300, 8, M, 'se', seed=29)
    Z = w['Xc'].copy()
    Z[M - 1] = w['X'][3]                             # the one live column of workgroup 96: on an observation
    Z[17, 2] = np.nan
    e = _engine(w)
    r1 = _run(e, w, Z, 10, 1, label='edge')
    assert r1['bound_kernel'] == 'mfma'
    d1 = r1['dots']
    assert np.isnan(d1[17]) and np.isnan(d1).sum() == 1 and np.isfinite(d1[M - 1])
    r0 = _run(e, w, Z, 10, 0, label='edge')
    _agree(r0, r1, w, 'edge')
    print('edge: last column |dot_mfma - dot_generic| %.3e' % abs(d1[M - 1] - r0['dots'][M - 1]))
    # an infinite coordinate makes the guard decline; forced past it (not through check_sweep, whose ub >= acq wants a number
    # where the value is one): NaN, as before -- nothing finite -- and the finite candidates keep their bits
    Z[4000, 7] = np.inf
    e.set_option('prune_bound', 1)
    e.sweep('ei', e.mean_at_obs()[1], Z, k=10, want_all=False)
    r = e.prune_report(vectors=False)
    assert r['bound_kernel'] == 'mfma' and r['guard'] == np.inf and r['path'] in ('pruned', 'fell back')
    di = e.prune_dots()
    assert np.isnan(di[4000]) and np.isnan(di[17])
    keep = np.ones(M, dtype=bool)
    keep[4000] = False
    assert np.array_equal(di[keep], d1[keep], equal_nan=True)
    e.close()
