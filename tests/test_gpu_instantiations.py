"""Every template case the size-selecting launchers can choose, run once at the smallest shape that reaches it (case lists and rules:
tests/inst_cases.py; that the lists reach every instantiation the library holds: tests/test_instantiation_cases_cpu.py; the bound
kernels' cases: the second parametrisation of tests/test_gpu_prune_bound_mfma.py and test_gpu_prune_bound_f32.py).

  k_rff_mfma5<JF, NSUB, DB>   n = 1 .. 128 features at d = 3, 9, 16, 17, 32 against a long-double reference
  k_path_update<KID, NJB>     S = 17, 33, 48, 81 draws of every covariance against tests/path_ref.py
  k_tri_matvec_rb<MBT, 4>     predict-with-gradients at N = 300: single points at d = 1 .. 15, two-pass batches of 1 .. 16 points,
                              one-pass batches at d = 1, 2, 3, with 128-column segments and the default

Each test prints its largest error / tolerance ratio (-s); profiles/instantiation_coverage.md records them."""
import numpy as np
import pytest

import inst_cases as ic
import path_ref
from oracle import gp_ref
from helpers import mu_tol, s2_tol, synth_problem

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# k_rff_mfma5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', ic.RFF_DS)
def test_the_thompson_sweep_at_every_feature_count_against_long_double(d):
    """Engine.rff_sweep at n = 1 .. 128 (S = 3; S = 1 at n = 8, 24, 100), M = 300 candidates, on a handle fitted at N = 5.

    reference   bias + sum_j theta_j cos(w_j . z + b_j) in numpy.longdouble (inst_cases.rff_reference);
    tolerance   sum_j |theta_j| (gamma_{d+1} (|b_j| + sum |w z|) + COS_POLY_ABS + |n_j| C3 + 2 u) + gamma_n sum |theta| + 2 u |bias|
                with the constants of tests/devmath_ref.py: the bound test_thompson_value_of_both_cosines_agrees_on_a_realistic_draw
                derives, one-sided because the reference is exact (inst_cases.rff_tol; at most 1e-12 max(1, sum |theta| + |bias|),
                and 100 times smaller than what any of four defects changes: tests/test_instantiation_cases_cpu.py);
    order       top_idx is gp_ref.topk_desc of the device's own values, top_val those values;
    witness     the single-buffer kernel (option x_rff = 1) agrees within twice the tolerance;
    slots       a candidate's bits depend on neither its slot nor M: the sweep over a permutation of the candidates and over the
                first 129 returns the same bits per candidate (k_rff_mfma5<JF >= 1, NSUB >= 1> used to miss this: it added a row's
                remainder-column terms into a different quad of the 16-lane reduction for every row of a lane group);
    NaN         at S = 1: a NaN coordinate makes its candidate's value NaN and changes no other candidate's bits.
    The failures of all n are collected, so one run names every bad (JF, NSUB, DB)."""
    from pybo_amd._lib import Engine
    rng = np.random.RandomState(d)
    X5 = rng.rand(5, d)
    Z = ic.rff_candidates(d)
    perm = np.random.RandomState(7).permutation(ic.RFF_M)
    e = Engine(0)
    e.fit(X5, np.sin(X5.sum(1)), 'se', np.full(d, 0.7 * np.sqrt(d)), 1.0, 1e-3, ic.RFF_BIAS)
    fails, kept, worst, worst_w = [], {}, 0.0, 0.0
    try:
        for n, S in ic.rff_cases(d):
            tag = 'n=%d S=%d <JF,NSUB,DB>=%s' % ((n, S) + (ic.rff5_case(n, d),))
            W, b, theta = ic.rff_draws(n, d, S)
            ref = ic.rff_reference(W, b, theta, ic.RFF_BIAS, Z)
            tol = ic.rff_tol(W, b, theta, ic.RFF_BIAS, Z)
            r = e.rff_sweep(W, b, theta, ic.RFF_BIAS, Z, k=ic.RFF_K)
            v = r['vals']
            ratio = float(np.max(np.abs((v - ref).astype(float)) / tol))
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                fails.append('%s: error / tolerance %.3g' % (tag, ratio))
            for s in range(S):
                order = gp_ref.topk_desc(v[s], ic.RFF_K)
                if not (np.array_equal(r['top_idx'][s], order) and _bits(r['top_val'][s], v[s][order])):
                    fails.append('%s: top-k of draw %d' % (tag, s))
            if not _bits(e.rff_sweep(W, b, theta, ic.RFF_BIAS, Z[perm], k=0)['vals'], v[:, perm]):
                fails.append('%s: a permutation of the candidates changes bits' % tag)
            if not _bits(e.rff_sweep(W, b, theta, ic.RFF_BIAS, Z[:129], k=0)['vals'], v[:, :129]):
                fails.append('%s: the first 129 candidates alone differ in bits' % tag)
            if S == 1:                               # a NaN coordinate poisons its candidate alone (rows 4 apart share the 4x4x4 tail's lanes)
                Zn = Z.copy()
                Zn[9, d - 1] = np.nan
                vn = e.rff_sweep(W, b, theta, ic.RFF_BIAS, Zn, k=0)['vals']
                if not (np.isnan(vn[0, 9]) and _bits(np.delete(vn, 9, axis=1), np.delete(v, 9, axis=1))):
                    fails.append('%s: a NaN candidate reaches %d others' % (tag, int(np.isnan(vn).sum()) - 1))
            kept[(n, S)] = (W, b, theta, v, tol)
        e.set_option('x_rff', 1)                     # process-wide
        try:
            for (n, S), (W, b, theta, v, tol) in kept.items():
                w = e.rff_sweep(W, b, theta, ic.RFF_BIAS, Z, k=0)['vals']
                ratio = float(np.max(np.abs(w - v) / (2.0 * tol)))
                worst_w = max(worst_w, ratio)
                if not ratio <= 1.0:
                    fails.append('n=%d S=%d %s: |witness - kernel| / (2 tolerance) %.3g' % (n, S, ic.rff5_case(n, d), ratio))
        finally:
            e.set_option('x_rff', 0)
    finally:
        e.close()
    print('k_rff_mfma5 d=%d: max error / tolerance %.3g, max |witness - kernel| / (2 tolerance) %.3g' % (d, worst, worst_w))
    assert not fails, '\n'.join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# k_path_update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', path_ref.KERNELS)
@pytest.mark.parametrize('case', ic.PATH_CASES)
def test_pathwise_sweeps_with_two_and_three_draw_blocks(case, kernel):
    """gpx_path_sweep at S = 17, 33, 48 (NJB = 2, 3, 3) and 81 (a full group, then NJB = 2), n = 100: the values within
    path_ref.value_tol of path_ref.values; the top-k as in test_sweep_values_topk_and_the_device_variant; draws 16, 32, 47 of the 48 and
    draw 80 of the 81, each swept alone (NJB = 1, the case tests/test_gpu_path.py holds), return the bits they have in the full call."""
    from test_gpu_path import CASES, _cands, _draws, _engine, _model
    N, d = CASES[case][:2]
    m = _model(case, kernel)
    Xc = _cands(d)
    e = _engine(m)
    worst = 0.0
    try:
        for S in ic.PATH_SS:
            D = _draws(m, ic.PATH_N, S, 7)
            out = e.path_sweep(D['W'], D['b'], D['theta'], D['v'], m['bias'], Xc, k=10)
            f, B = path_ref.values(kernel, m['X'], m['ell'], m['rho'], m['bias'], D['W'], D['b'], D['theta'], D['v'], Xc)
            tol = path_ref.value_tol(B, f, N, ic.PATH_N, m['rho'])
            err = np.abs(out['vals'] - f)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (case, kernel, S, ic.path_njb(S), float((err / tol).max()))
            for s in range(S):
                order = gp_ref.topk_desc(out['vals'][s], 10)
                assert np.array_equal(out['top_idx'][s], order) and _bits(out['top_val'][s], out['vals'][s][order]), (S, s)
            for q in ic.PATH_ALONE.get(S, ()):
                sel = slice(q, q + 1)
                alone = e.path_sweep(D['W'][sel], D['b'][sel], D['theta'][sel], D['v'][sel], m['bias'], Xc, k=0)['vals']
                assert _bits(alone[0], out['vals'][q]), (case, kernel, S, q)
    finally:
        e.close()
    print('k_path_update %s %s: max error / tolerance %.3g' % (case, kernel, worst))


# ---------------------------------------------------------------------------------------------------------------------
# k_tri_matvec_rb
# ---------------------------------------------------------------------------------------------------------------------
def _grad_pair(d, kernel, npts):
    """The model (N = 300, Np = 384), its oracle, and npts queries: one on an observation, one on the last real row (its neighbours in
    the factor are the identity padding)."""
    X, y, ell = synth_problem(ic.GRAD_N, d, seed=31 + d)
    rho, sn2, bias = 1.3, 1e-3, 0.2
    ref = gp_ref.make_gp(sn2, rho, ell, bias, kernel)
    ref.add_data(X, y)
    from pybo_amd._lib import Engine
    e = Engine(0)
    e.fit(X, y, kernel, ell, rho, sn2, bias)
    Z = np.random.RandomState(8).rand(npts, d)
    Z[3] = X[5]
    Z[npts - 1] = X[ic.GRAD_N - 1]
    return e, ref, rho, Z


def _predict(e, Z, form, kern, cs):
    e.set_option('grad_form', form)
    e.set_option('grad_kernel', kern)
    e.set_option('grad_rb_cs', cs)
    return e.predict(Z, grad=True)


def _against_oracle(got, want, rho, label):
    """mu_tol, s2_tol, rtol 1e-6 / atol 1e-8 on the gradients; returns the largest error / tolerance."""
    tols = (mu_tol(want[0], rho), s2_tol(want[1], rho), 1e-6 * np.abs(want[2]) + 1e-8, 1e-6 * np.abs(want[3]) + 1e-8)
    worst = 0.0
    for j in range(4):
        ratio = float(np.max(np.abs(got[j] - want[j]) / tols[j]))
        assert ratio <= 1.0, (label, j, ratio)
        worst = max(worst, ratio)
    return worst


def _close(a, b, want, label):
    """Two forms of the same four results: within 2e-9 max |want| each."""
    for j in range(4):
        scale = np.abs(want[j]).max()
        assert np.all(np.abs(a[j] - b[j]) <= 2e-9 * scale), (label, j, float(np.max(np.abs(a[j] - b[j]))), scale)


def _rows(results):
    return [np.concatenate([r[j] for r in results]) for j in range(4)]


@pytest.mark.parametrize('kernel', ic.GRAD_KERNELS)
@pytest.mark.parametrize('d', ic.GRAD_SINGLE_DS)
def test_single_point_gradients_at_every_dimension_of_the_one_pass_form(d, kernel):
    """Single points at d = 1 .. 15: one pass over T with MBT = 1 + d = 2 .. 16 right-hand sides, with 128-column segments (three at
    N = 300: rows that cross a segment edge take the masked piece, the last segment is partial) and the default (one segment).  Against
    the oracle at the tolerances of test_single_point_gradients_take_one_pass_over_the_inverse; against grad_kernel = 0
    (k_tri_matvec_multi) within 2e-9 max |want|; the rows of a one-pass batch (grad_form = 2) are the single points' bits.  The two
    segment widths agree within 2e-9 max |want|, not in bits: a lane adds its columns 2 l, 2 l + 128, 2 l + 256 of one 2048-column
    segment before the lanes are summed, and the three 128-column segments are summed over the lanes first and added afterwards."""
    e, ref, rho, Z = _grad_pair(d, kernel, 7)
    try:
        want = ref.predict(Z, grad=True)
        base = _predict(e, Z, 1, 0, 0)
        _against_oracle(base, want, rho, 'k_tri_matvec_multi')
        by_cs = {}
        for cs in ic.GRAD_CS:
            singles = _rows([_predict(e, Z[i:i + 1], 0, -1, cs) for i in range(len(Z))])
            worst = _against_oracle(singles, want, rho, (d, kernel, cs))
            _close(singles, base, want, ('one pass against k_tri_matvec_multi', d, kernel, cs))
            batch = _predict(e, Z, 2, -1, cs)
            for j in range(4):
                assert _bits(batch[j], singles[j]), ('one-pass batch against single points', d, kernel, cs, j)
            by_cs[cs] = singles
            print('k_tri_matvec_rb<%d,4> %s cs=%d: max error / tolerance %.3g' % (1 + d, kernel, cs, worst))
        _close(by_cs[ic.GRAD_CS[0]], by_cs[ic.GRAD_CS[1]], want, ('segment widths', d, kernel))
    finally:
        e.close()


@pytest.mark.parametrize('kernel', ic.GRAD_KERNELS)
def test_two_pass_gradients_at_every_batch_size_of_the_register_blocked_kernel(kernel):
    """Batches of 1 .. 16 points at d = 3 under grad_form = 1, grad_kernel = 1: MBT = mb on T (mode 0) and on U (mode 1, the masks of
    the upper triangle), both segment widths.  Against the oracle, against k_tri_matvec_multi within 2e-9 max |want|, and every row has
    the bits it has in the batch of 16, whatever batch it travels in (also as the last row of a batch)."""
    d = ic.GRAD_TWO_PASS_D
    e, ref, rho, Z = _grad_pair(d, kernel, 16)
    try:
        want = ref.predict(Z, grad=True)
        base = _predict(e, Z, 1, 0, 0)
        by_cs = {}
        for cs in ic.GRAD_CS:
            full = _predict(e, Z, 1, 1, cs)
            worst = _against_oracle(full, want, rho, (kernel, cs))
            _close(full, base, want, ('register-blocked against k_tri_matvec_multi', kernel, cs))
            for mb in ic.GRAD_TWO_PASS_MB:
                head = _predict(e, Z[:mb], 1, 1, cs)
                tail = _predict(e, Z[16 - mb:], 1, 1, cs)
                for j in range(4):
                    assert _bits(head[j], full[j][:mb]) and _bits(tail[j], full[j][16 - mb:]), ('batch of', mb, kernel, cs, j)
            by_cs[cs] = full
            print('k_tri_matvec_rb two-pass %s cs=%d: max error / tolerance %.3g' % (kernel, cs, worst))
        _close(by_cs[ic.GRAD_CS[0]], by_cs[ic.GRAD_CS[1]], want, ('segment widths', kernel))
    finally:
        e.close()


@pytest.mark.parametrize('kernel', ic.GRAD_KERNELS)
@pytest.mark.parametrize('d', ic.GRAD_ONE_PASS_DS)
def test_one_pass_batches_at_every_product_of_points_and_right_hand_sides(d, kernel):
    """Batches of 1 .. 16 // (1 + d) points under grad_form = 2 at d = 1, 2, 3: MBT = mb (1 + d), the products the single points do not
    give twice over, and one batch longer than a pass (two chunks).  Every row has the single point's bits; against the oracle and
    k_tri_matvec_multi as above."""
    chunk = ic.GB // (1 + d)
    e, ref, rho, Z = _grad_pair(d, kernel, chunk + 2)
    try:
        want = ref.predict(Z, grad=True)
        base = _predict(e, Z, 1, 0, 0)
        for cs in ic.GRAD_CS:
            singles = _rows([_predict(e, Z[i:i + 1], 2, -1, cs) for i in range(len(Z))])
            worst = _against_oracle(singles, want, rho, (d, kernel, cs))
            _close(singles, base, want, ('one pass against k_tri_matvec_multi', d, kernel, cs))
            for M in list(range(1, chunk + 1)) + [chunk + 2]:
                got = _predict(e, Z[:M], 2, -1, cs)
                for j in range(4):
                    assert _bits(got[j], singles[j][:M]), ('batch of', M, d, kernel, cs, j)
            print('k_tri_matvec_rb one-pass batches d=%d %s cs=%d: max error / tolerance %.3g' % (d, kernel, cs, worst))
    finally:
        e.close()
