"""The bound pass of a selection-only sweep in fp32 on the matrix pipe with a per-candidate margin (k_bound_mfma32, csrc/bound_f32.h,
DESIGN.md section 2.1): the kernel writes dot_hi >= alpha2 . k(X, z_n), and everything downstream is sound for any such value.

Held here, at the shapes of tests/test_gpu_prune_bound_mfma.py with the kernel forced (diagnostic option prune_bound = 2):

  soundness   every invariant of tests/test_gpu_prune_bound.py (check_sweep), the top-k array_equal to prune = 0 included; the report
              names kernel 2 and carries E;
  margin      for every candidate, against the fp64 matrix-pipe kernel's dots (prune_bound = 1) of the same engine, whose own error
              is eps_k rho S (tests/test_gpu_prune_bound_mfma.py):
                  dots32 >= dots64 - eps_k rho S          dots32 - dots64 <= 2 E B_n + eps_k rho S,
              B_n = sum |w_i| k_i from numpy with alpha~ = T^T a from the device's T and a (taken 1e-9 larger: numpy's own rounding;
              the flush term F < 1e-30 (rho S + Np) is not added: the assertion is stricter than the proof), E from the report;
              NaN where and only where the fp64 dots are NaN;
  edges       a candidate on an observation, one with a NaN coordinate, one 100 length scales away;
  guards      under -1 the fp32 kernel runs from 131072 candidates on and not below (bit for bit the fp64 kernel there); one
              candidate moved until the guards decline -- first the fp64 guard alone, then E > 2^-10 as well: at these N the second
              implies the first (E reaches 2^-10 near (d + 4)(R_x + R_z)^2 = 2^15 (d + 4) / (d + 5), so it binds alone only from
              Np ~ 27000 to 30000 on) -- gives the dots of the kernel that runs instead, array_equal; a weight that is subnormal in
              fp32 refuses the fp32 kernel alone, and the fp64 matrix-pipe kernel runs: its dots, array_equal;
  elsewhere   Matern-5/2 and d = 19: the generic kernel under every value;
  second bound and ensemble   one check_rows case (tests/test_gpu_prune_rows.py) and one 3-member ensemble under prune_bound = 2."""
import numpy as np
import pytest

import inst_cases as ic
from test_gpu_prune import _dev
from test_gpu_prune_bound import _engine, _expected_sizes, _problem, check_sweep
from test_gpu_prune_bound_mfma import DS, MS, NS, _eps_k

pytestmark = pytest.mark.gpu

G = 4096
E_MAX = 2.0 ** -10
F32_MIN_M = 131072


def _weights(e, w):
    """|w_i| = rho |alpha~_i|, alpha~ = T^T a from the device's factor inverse and a."""
    T, a = e.get_matrix('T'), e.get_vectors()[0]
    return np.abs(T.T @ a)


def _B(w, absw, Z):
    """B_n = sum_i |w_i| k(x_i, z_n) in fp64 (the expansion of the distances: its 1e-13 relative error is nothing beside the 1e-9 below)."""
    inv = 1.0 / w['ell']
    Xs, Zs = w['X'] * inv, np.nan_to_num(Z * inv, nan=0.0, posinf=1e150, neginf=-1e150)
    out = np.empty(len(Z))
    x2 = (Xs ** 2).sum(1)
    for j0 in range(0, len(Z), 8192):
        z = Zs[j0:j0 + 8192]
        r2 = np.maximum(x2[:, None] + (z ** 2).sum(1)[None, :] - 2.0 * (Xs @ z.T), 0.0)
        out[j0:j0 + 8192] = absw @ (w['rho'] * np.exp(-0.5 * r2))
    return out * (1.0 + 1e-9)


def _dots(e, w, Z, k, bound):
    """One pruned sweep with the bound pass's kernel forced; (report, dots)."""
    e.set_option('prune', 1)
    e.set_option('prune_bound', bound)
    dZ = _dev(Z)
    e.sweep_dev('ei', e.mean_at_obs()[1], dZ.data_ptr(), len(Z), k)
    r = e.prune_report(vectors=False)
    return r, e.prune_dots()


def _margin(e, w, Z, r32, d32, label):
    """dots32 against the fp64 matrix-pipe kernel's dots, every candidate."""
    r64, d64 = _dots(e, w, Z, 10, 1)
    assert r64['bound_kernel'] == 'mfma' and np.isnan(r64['E']), label
    assert np.array_equal(np.isnan(d32), np.isnan(d64)), label
    ok = ~np.isnan(d64)
    E = r32['E']
    assert 0.0 < E < 0.5, (label, E)
    room = _eps_k(w['d'], r64['guard']) * w['rho'] * r64['S']
    B = _B(w, _weights(e, w), Z)
    low = d32[ok] - d64[ok]
    print('%-30s E %.3e  min (d32 - d64) %.3e  max (d32 - d64) / (2 E B) %.4f  eps_k rho S %.3e' %
          (label, E, float(low.min()), float(np.max(low / (2.0 * E * B[ok] + 1e-300))), room))
    assert np.all(low >= -room), (label, float(low.min()), room)
    assert np.all(low <= 2.0 * E * B[ok] + room), (label, float(np.max(low - 2.0 * E * B[ok])), room)
    assert r32['S'] == r64['S'] and r32['delta'] == r64['delta'], label


@pytest.mark.parametrize('N,d,M', [(N, d, MS[(i + j) % 3]) for i, N in enumerate(NS) for j, d in enumerate(DS)])
def test_bound_invariants_and_margin_with_the_fp32_kernel(N, d, M):
    w = _problem(N, d, M, 'se', seed=7 * N + d)
    e = _engine(w)
    label = 'N=%d d=%d M=%d' % (N, d, M)
    e.set_option('prune_bound', 2)
    r = check_sweep(e, w, w['Xc'], 10, prune=1, label=label + ' bound=2')
    assert r['path'] in ('pruned', 'fell back') and r['bound_kernel'] == 'mfma32', (label, r['bound_kernel'])
    _margin(e, w, w['Xc'], r, e.prune_dots(), label)
    e.close()


@pytest.mark.parametrize('N,d', [(N, d) for N in ic.BOUND_NS for d in ic.BOUND_DS])
def test_bound_invariants_and_margin_at_the_template_cases_the_shapes_above_do_not_reach(N, d):
    """k_bound_mfma32<KS, NC, false> at d = 3, 4 (1, NC), 5, 6 (2, -), 11, 12 (3, NC), 13, 14 (4, -), 17, 18 (5, -): the same body
    (tests/inst_cases.py, tests/test_instantiation_cases_cpu.py: with DS these reach every instantiation)."""
    test_bound_invariants_and_margin_with_the_fp32_kernel(N, d, 3 * G + 1)


def test_a_candidate_on_an_observation_a_nan_one_and_a_far_one():
    M, k = 3 * G + 77, 10
    w = _problem(300, 3, M, 'se', seed=51)
    Z = w['Xc'].copy()
    Z[5] = w['X'][7]                       # exponent 0 up to cancellation: it may come out above 0, inside the margin
    Z[9, 1] = np.nan
    Z[11] = 50.0                           # 100 length scales away: every covariance is flushed, dot_hi is the flush term
    e = _engine(w)
    e.set_option('prune_bound', 2)
    r = check_sweep(e, w, Z, k, prune=1, label='edges bound=2')
    d32 = e.prune_dots()
    assert r['bound_kernel'] == 'mfma32'
    assert np.isnan(d32[9]) and np.isnan(r['ub_kept'][9]) and (9 in r['seed_idx'] or 9 in r['idx'])
    assert np.isfinite(d32[5]) and 0.0 <= d32[11] <= 1e-30 * (w['rho'] * r['S'] + 384)
    _margin(e, w, Z, r, d32, 'edges')
    e.close()


def test_the_size_rule_and_the_guards_choose_the_kernel():
    N, d, k = 1024, 2, 10
    w = _problem(N, d, F32_MIN_M, 'se', seed=61)
    e = _engine(w)
    Z = w['Xc']
    target = e.mean_at_obs()[1]

    def topk(Zc, prune, bound):
        e.set_option('prune', prune)
        e.set_option('prune_bound', bound)
        dZ = _dev(Zc)
        return e.sweep_dev('ei', target, dZ.data_ptr(), len(Zc), k)

    # below 131072 candidates the default is the fp64 kernel, bit for bit
    rs, ds = _dots(e, w, Z[:40961], k, -1)
    r1, d1 = _dots(e, w, Z[:40961], k, 1)
    assert rs['bound_kernel'] == 'mfma' and np.isnan(rs['E']) and np.array_equal(ds, d1)
    # from 131072 on, the fp32 kernel by its guards
    plain = topk(Z, 0, -1)
    rg, dg = _dots(e, w, Z, k, -1)
    assert rg['bound_kernel'] == 'mfma32' and 0.0 < rg['E'] <= E_MAX and rg['guard'] <= N, rg
    got = topk(Z, 1, -1)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    r2, d2 = _dots(e, w, Z, k, 2)
    assert np.array_equal(dg, d2)
    # one candidate moved until the fp64 guard declines (E still small), then until E > 2^-10 as well: the generic kernel's dots
    for where, e_over in ((10.0, False), (400.0, True)):
        Zf = Z.copy()
        Zf[F32_MIN_M // 2] = where
        rf, df = _dots(e, w, Zf, k, -1)
        assert rf['guard'] > N and (rf['E'] > E_MAX) == e_over, (where, rf['guard'], rf['E'])
        assert rf['bound_kernel'] == 'generic', (where, rf['bound_kernel'])
        r0, d0 = _dots(e, w, Zf, k, 0)
        assert np.array_equal(df, d0, equal_nan=True), where
        got, plain = topk(Zf, 1, -1), topk(Zf, 0, -1)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), where
    e.close()


def test_a_weight_subnormal_in_fp32_hands_the_pass_to_the_fp64_matrix_pipe_kernel():
    """The link "fp32 considered and refused -> k_bound_mfma": the observations' spread about the bias scaled by 1e-40 scales every weight
    w_i = rho alpha~_i by as much, so some are subnormal in fp32; the radii and E do not change, so the weight guard alone refuses."""
    N, d, k = 1024, 2, 10
    w = _problem(N, d, F32_MIN_M, 'se', seed=61)
    w['y'], w['bias'] = 1e-40 * (w['y'] - w['bias']), 0.0        # (a bias of 0: beside 0.2 the scaled spread would round away)
    e = _engine(w)
    absw = w['rho'] * _weights(e, w)
    assert np.any((absw > 0.0) & (absw < 2.0 ** -126)), (absw.min(), absw.max())
    rg, dg = _dots(e, w, w['Xc'], k, -1)
    assert rg['bound_kernel'] == 'mfma' and 0.0 < rg['E'] <= E_MAX and rg['guard'] <= N, rg
    r1, d1 = _dots(e, w, w['Xc'], k, 1)
    assert r1['bound_kernel'] == 'mfma' and np.isnan(r1['E']) and np.array_equal(dg, d1)
    e.close()


@pytest.mark.parametrize('kernel,d', [('matern5', 4), ('se', 19)])
def test_other_covariances_and_long_inner_products_keep_the_generic_kernel(kernel, d):
    M, k = 3 * G + 5, 10
    w = _problem(300, d, M, kernel, seed=71)
    e = _engine(w)
    ref = None
    for bound in (2, 1, -1, 0):
        r, dots = _dots(e, w, w['Xc'], k, bound)
        assert r['bound_kernel'] == 'generic' and np.isnan(r['guard']) and np.isnan(r['E']), (kernel, d, bound)
        assert ref is None or np.array_equal(dots, ref)
        ref = dots
    e.set_option('prune_bound', 2)
    check_sweep(e, w, w['Xc'], k, prune=1, truth=False, label='%s d=%d bound=2' % (kernel, d))
    e.close()


def test_the_second_bound_reads_the_fp32_dots():
    from test_gpu_prune_rows import _scaled, _truth, check_rows
    N, k = 4096, 10
    M = 3 * _expected_sizes(N, k, 1 << 20)[0] + 1000
    w = _scaled(N, M, 0.5, N)
    e = _engine(w)
    e.set_option('prune_bound', 2)
    target = e.mean_at_obs()[1]
    r = check_rows(e, w, _truth(e, w['Xc'], target), target, k, 16, label='N=4096 rows=16 bound=2')
    assert r['path'] == 'pruned' and r['nR'] == 16 and r['bound_kernel'] == 'mfma32'
    e.close()


def test_the_ensemble_sweep_with_the_fp32_kernel_on_every_member():
    from test_gpu_ens_prune import _ensemble, _same, _sweep
    p, engines = _ensemble('se_n3')
    try:
        plain = _sweep(p, engines, p['Z'], 10, 0)
        for e in engines:
            e.set_option('prune_bound', 1)
        ref = _sweep(p, engines, p['Z'], 10, 1)
        for e in engines:
            e.set_option('prune_bound', 2)
        pruned = _sweep(p, engines, p['Z'], 10, 1)
        assert _same(plain, pruned) and _same(plain, ref)
        assert plain[3]['path'] == 'plain' and pruned[3]['path'] == 'pruned' and pruned[2] < 1.0
        # the members report no kernel of their own: that theirs was the fp32 one shows in the ensemble bound, which carries the
        # members' margins E B_n (1e-6 of B_n and more) above the bound from the fp64 dots (whose own error is 1e-13 of rho S)
        ub32, ub64 = pruned[3]['ub'], ref[3]['ub']
        both = np.isfinite(ub32) & np.isfinite(ub64) & (ub64 > 0.0)
        above = float(np.mean(ub32[both] > ub64[both]))
        print('ensemble: bound from the fp32 dots above the one from the fp64 dots on %.4f of %d candidates' % (above, int(both.sum())))
        assert both.sum() > 0 and above > 0.5, above
    finally:
        for e in engines:
            e.set_option('prune_bound', -1)
