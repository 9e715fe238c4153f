"""The bound pass of a selection-only sweep with its distances on the matrix pipe (k_bound_mfma).

For the SE-ARD covariance up to d = 18 the dots alpha2 . k(X, z_n) come from an inner-product form of the exponent whose
cancellation the direct differences of k_sweep_rankq<1> do not have.  Held here:

  soundness   every invariant of tests/test_gpu_prune_bound.py (check_sweep) with the matrix-pipe kernel forced (diagnostic
              option prune_bound = 1), the generic one forced (0) and the guard choosing (-1); the report says which ran;
  guard       the report's (d + 4)(R_x + R_z)^2 against numpy's from the same centre (the midpoint of the scaled
              observations' box), and the choice: matrix pipe <=> that value <= Np;
  agreement   the two kernels' dots (gpx_prune_dots, kept under prune_keep before EI is taken) differ by at most
              eps_k rho S, eps_k = u ((d + 4)(R_x + R_z)^2 + 3): the exponent's absolute error, which is the covariance's
              relative one (entries <= rho), plus one rounding each for rho alpha2, for the exponential and for the product
              with rho that the weights took over; S from the report.  The summation orders of the two kernels differ as
              well (worst case (N / 8 + Np / 16 + 17) u rho ||alpha2||_1, part of delta's budget): NOT added, the
              assertion is stricter than the proof;
  edges       a candidate on an observation, one with a NaN coordinate, one far outside the data;
  switch      one candidate moved until the guard declines: the generic kernel runs, the top-k is that of prune = 0;
  elsewhere   Matern-5/2 and d = 19: the generic kernel whatever the option says.

check_sweep asserts the pruned top-k array_equal to the plain one in every case."""
import numpy as np
import pytest

import inst_cases as ic
from oracle import gp_ref
from test_gpu_prune_bound import _engine, _problem, check_sweep

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
G = 4096                                   # seeds at every N here (tests/test_gpu_prune_bound.py: _expected_sizes)
MS = (3 * G, 3 * G + 1, 40961)
NS = (128, 130, 1024, 2049)
DS = (1, 2, 8, 9, 16)


def _guard_numpy(w, Z):
    """(d + 4)(R_x + R_z)^2 as k_bound_centre / k_bound_aug / k_bound_rz form it; rows with a NaN are not recorded."""
    inv = 1.0 / w['ell']
    Xs, Zs = w['X'] * inv, Z * inv
    c = 0.5 * Xs.min(0) + 0.5 * Xs.max(0)
    rx = np.sqrt(((Xs - c) ** 2).sum(1).max())
    z2 = ((Zs - c) ** 2).sum(1)
    rz = np.sqrt(np.nanmax(z2))
    return (w['d'] + 4) * (rx + rz) ** 2


def _eps_k(d, guard):
    return U53 * (guard + 3.0)


def _run(e, w, Z, k, bound, prune=1, label=''):
    e.set_option('prune_bound', bound)
    r = check_sweep(e, w, Z, k, prune=prune, label='%s bound=%d' % (label, bound))
    r['dots'] = e.prune_dots() if r['path'] in ('pruned', 'fell back') else None
    return r


def _agree(r0, r1, w, label):
    """generic (r0) against matrix pipe (r1): the dots within eps_k rho S, NaN where and only where the other is."""
    d0, d1 = r0['dots'], r1['dots']
    assert np.array_equal(np.isnan(d0), np.isnan(d1)), label
    ok = ~np.isnan(d0)
    bound = _eps_k(w['d'], r1['guard']) * w['rho'] * r1['S']
    diff = float(np.max(np.abs(d0[ok] - d1[ok])))
    print('%-34s max |dot_mfma - dot_generic| %.3e  eps_k rho S %.3e  (guard %.4g)' % (label, diff, bound, r1['guard']))
    assert diff <= bound, (label, diff, bound)
    assert r0['S'] == r1['S'] and r0['delta'] == r1['delta'], label


@pytest.mark.parametrize('N,d,M', [(N, d, MS[(i + j) % 3]) for i, N in enumerate(NS) for j, d in enumerate(DS)])
def test_bound_invariants_with_either_kernel_and_with_the_guard(N, d, M):
    w = _problem(N, d, M, 'se', seed=7 * N + d)
    Np = (N + 127) // 128 * 128
    e = _engine(w)
    label = 'N=%d d=%d M=%d' % (N, d, M)
    gv = _guard_numpy(w, w['Xc'])
    r1 = _run(e, w, w['Xc'], 10, 1, label=label)
    assert r1['bound_kernel'] == 'mfma' and abs(r1['guard'] - gv) <= 1e-10 * gv, (label, r1['guard'], gv)
    r0 = _run(e, w, w['Xc'], 10, 0, label=label)
    assert r0['bound_kernel'] == 'generic' and np.isnan(r0['guard']), label
    rg = _run(e, w, w['Xc'], 10, -1, label=label)
    assert abs(rg['guard'] - gv) <= 1e-10 * gv, label
    if abs(gv - Np) > 1e-9 * Np:
        assert rg['bound_kernel'] == ('mfma' if gv <= Np else 'generic'), (label, gv, Np)
    assert np.array_equal(rg['dots'], (r1 if rg['bound_kernel'] == 'mfma' else r0)['dots'], equal_nan=True), label
    assert r0['path'] in ('pruned', 'fell back') and r1['path'] in ('pruned', 'fell back')
    _agree(r0, r1, w, label)
    e.close()


@pytest.mark.parametrize('N,d', [(N, d) for N in ic.BOUND_NS for d in ic.BOUND_DS])
def test_bound_invariants_at_the_template_cases_the_shapes_above_do_not_reach(N, d):
    """k_bound_mfma<KS, NC> at d = 3, 4 (1, NC), 5, 6 (2, -), 11, 12 (3, NC), 13, 14 (4, -), 17, 18 (5, -): the same body (tests/inst_cases.py,
    tests/test_instantiation_cases_cpu.py: with DS these reach every instantiation)."""
    test_bound_invariants_with_either_kernel_and_with_the_guard(N, d, 3 * G + 1)


def test_a_candidate_on_an_observation_a_nan_one_and_a_far_one():
    M, k = 3 * G + 77, 10
    w = _problem(300, 3, M, 'se', seed=51)
    Z = w['Xc'].copy()
    Z[5] = w['X'][7]                       # exponent exactly 0 up to cancellation: limited to <= 0
    Z[9, 1] = np.nan
    Z[11] = 50.0                           # 100 length scales away: the covariance underflows
    e = _engine(w)
    r1 = _run(e, w, Z, k, 1, label='edges')
    assert r1['bound_kernel'] == 'mfma'
    assert np.isnan(r1['dots'][9]) and np.isnan(r1['ub_kept'][9]) and (9 in r1['seed_idx'] or 9 in r1['idx'])
    assert np.isfinite(r1['dots'][5]) and r1['dots'][11] == 0.0
    r0 = _run(e, w, Z, k, 0, label='edges')
    _agree(r0, r1, w, 'edges')
    # the candidate on the observation alone, at the radius of the data (the far candidate inflates eps_k above)
    rho, S = w['rho'], r1['S']
    assert abs(r1['dots'][5] - r0['dots'][5]) <= _eps_k(3, _guard_numpy(w, w['Xc'])) * rho * S
    e.close()


def test_the_guard_declines_when_one_candidate_is_far_and_the_generic_kernel_runs():
    M, k, N, d = 3 * G + 5, 10, 1024, 2
    w = _problem(N, d, M, 'se', seed=61)
    e = _engine(w)
    r = _run(e, w, w['Xc'], k, -1, label='near')
    assert r['bound_kernel'] == 'mfma' and r['guard'] <= 0.5 * N
    Z = w['Xc'].copy()
    Z[M // 2] = 30.0                       # (d + 4)(R_x + R_z)^2 > 6 * 60^2 > Np
    gv = _guard_numpy(w, Z)
    assert gv > 2 * N
    rf = _run(e, w, Z, k, -1, label='one far')
    assert rf['bound_kernel'] == 'generic' and abs(rf['guard'] - gv) <= 1e-10 * gv
    r0 = _run(e, w, Z, k, 0, label='one far')
    assert np.array_equal(rf['dots'], r0['dots'], equal_nan=True)          # bit for bit today's kernel
    # an infinite coordinate: the radius is infinite, the guard declines
    Z[M // 3, 1] = np.inf
    ri = _run(e, w, Z, k, -1, label='one infinite')
    assert ri['bound_kernel'] == 'generic' and ri['guard'] == np.inf
    e.close()


@pytest.mark.parametrize('kernel,d', [('matern5', 4), ('se', 19)])
def test_other_covariances_and_long_inner_products_keep_the_generic_kernel(kernel, d):
    M, k = 3 * G + 5, 10
    w = _problem(300, d, M, kernel, seed=71)
    e = _engine(w)
    for bound in (1, -1, 0):
        r = _run(e, w, w['Xc'], k, bound, label='%s d=%d' % (kernel, d))
        assert r['bound_kernel'] == 'generic' and np.isnan(r['guard'])
    e.close()


def test_the_default_sweep_reports_its_kernel_and_plain_paths_report_none():
    M, k = 40961, 10
    w = _problem(1024, 2, M, 'se', seed=81)
    e = _engine(w)
    r = _run(e, w, w['Xc'], k, -1, prune=-1, label='auto')
    if r['path'] in ('pruned', 'fell back'):
        assert r['bound_kernel'] == 'mfma'
    else:
        assert r['bound_kernel'] is None
    e.set_option('prune', 0)
    e.sweep('ei', e.mean_at_obs()[1], w['Xc'][:5000], k=k, want_all=False)
    assert e.prune_report()['bound_kernel'] is None
    e.close()
