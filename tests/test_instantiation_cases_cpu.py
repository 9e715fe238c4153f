"""Every template case a launcher can choose has a test case, and every test case maps to a template case (no GPU needed).

The instantiations of the five size-selected kernel families are read from the host stubs of the built libgpx.so and held against what
the case lists of tests/inst_cases.py reach under the restated selection rules: a new template case without a test case fails here, and
so does a test case that maps to no instantiation.  The GPU side is tests/test_gpu_instantiations.py and the second parametrisation of
tests/test_gpu_prune_bound_mfma.py / test_gpu_prune_bound_f32.py; what the whole suite launches is recorded in
profiles/instantiation_coverage.md.

The Thompson inputs are checked as well: the tolerance of every case stays below what test_random_thompson_shapes_against_numpy grants
(a condition on the inputs -- the scale of W), and the reference recomputed with a defect misses the honest one by at least 100 times
the tolerance, so the tolerance cannot hide a dropped feature, exchanged weights or phases, or exchanged candidate rows."""
import os

import numpy as np
import pytest

import inst_cases as ic

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pybo_amd', 'csrc', 'libgpx.so')


@pytest.fixture(scope='module')
def inst():
    assert os.path.exists(LIB), 'build the library first (__graft_entry__.build())'
    return ic.kernel_instantiations(LIB)


def _b(v):
    return 'true' if v else 'false'


def test_the_thompson_cases_reach_exactly_the_instantiations_of_k_rff_mfma5(inst):
    reached = set()
    for d in ic.RFF_DS:
        for n, S in ic.rff_cases(d):
            case = ic.rff5_case(n, d)
            assert case is not None, (n, d)
            reached.add((str(case[0]), str(case[1]), _b(case[2])))
    assert reached == inst['k_rff_mfma5'], (sorted(reached - inst['k_rff_mfma5']), sorted(inst['k_rff_mfma5'] - reached))
    assert len(reached) == 48
    # dp = 4, 12, 16, 20, 32: odd and even counts of k-groups on either side of the DB boundary
    assert sorted({(d + 3) // 4 for d in ic.RFF_DS}) == [1, 3, 4, 5, 8]


def test_the_pathwise_cases_reach_exactly_the_instantiations_of_k_path_update(inst):
    reached, new = set(), set()
    for kernel in ic.KIDS:
        for S in ic.PATH_SS_BEFORE:
            reached |= ic.path_cases(kernel, S)
        for S in ic.PATH_SS:
            new |= ic.path_cases(kernel, S)
    assert {njb for _, njb in new} == {2, 3, 4} and {njb for _, njb in reached} == {1, 4}
    assert ic.path_njb(81) == [4, 2] and ic.path_njb(17) == [2] and ic.path_njb(33) == [3] and ic.path_njb(48) == [3]
    both = {(str(k), str(j)) for k, j in reached | new}
    assert both == inst['k_path_update'], (sorted(both - inst['k_path_update']), sorted(inst['k_path_update'] - both))
    for S, alone in ic.PATH_ALONE.items():
        assert S in ic.PATH_SS and all(0 <= q < S for q in alone)


def test_the_gradient_cases_reach_exactly_the_instantiations_of_k_tri_matvec_rb(inst):
    reached = set()
    for d, M, form, kern in ic.grad_calls():
        got = ic.tri_rb_cases(d, M, form, kern)
        assert got, (d, M, form, kern)
        reached |= got
    # every MBT on T (mode 0) and on U (mode 1): each has its own shuffle tree and store index, and mode 1 its own masks
    assert reached == {(mbt, mode) for mbt in range(1, 17) for mode in (0, 1)}
    lib = {(str(mbt), '4') for mbt, _ in reached}
    assert lib == inst['k_tri_matvec_rb'], (sorted(lib - inst['k_tri_matvec_rb']), sorted(inst['k_tri_matvec_rb'] - lib))
    # the one-pass lists alone give every product mb (1 + d) on T
    one = set()
    for d, M, form, kern in ic.grad_calls():
        if form != 1:
            one |= ic.tri_rb_cases(d, M, form, kern)
    assert {m for m, _ in one} == set(range(2, 17))


def test_the_bound_cases_reach_exactly_the_instantiations_of_both_bound_kernels(inst):
    from test_gpu_prune_bound_mfma import DS
    assert ic.BOUND_DS_BEFORE == DS
    ds = ic.BOUND_DS_BEFORE + ic.BOUND_DS
    assert sorted(ds) == list(range(1, 7)) + [8, 9] + list(range(11, 15)) + [16, 17, 18]
    reached = {ic.bound_case(d) for d in ds}
    assert {ic.bound_case(d) for d in ic.BOUND_DS_BEFORE} < reached
    f64 = {(str(ks), _b(nc)) for ks, nc in reached}
    assert f64 == inst['k_bound_mfma'], (sorted(f64 - inst['k_bound_mfma']), sorted(inst['k_bound_mfma'] - f64))
    # the factorised form takes KS alone: reached for KS = 1 .. 5 by the cases of tests/test_gpu_prune_bound_fact.py
    from test_gpu_prune_bound_fact import CASES
    fact = {(str(ic.bound_case(d)[0]), 'false', 'true') for d, N in CASES}
    f32 = {(ks, nc, 'false') for ks, nc in f64} | fact
    assert f32 == inst['k_bound_mfma32'], (sorted(f32 - inst['k_bound_mfma32']), sorted(inst['k_bound_mfma32'] - f32))
    assert len(f64) == 9 and len(fact) == 5


@pytest.mark.parametrize('d', ic.RFF_DS)
def test_the_thompson_inputs_discriminate_and_their_tolerance_is_capped(d):
    Z = ic.rff_candidates(d)
    weakest = np.inf
    for n, S in ic.rff_cases(d):
        W, b, theta = ic.rff_draws(n, d, S)
        assert len(np.unique(np.abs(theta[0]))) == n and np.all((b >= 0) & (b < 2 * np.pi)) and np.all(np.abs(Z) <= 1)
        tol = ic.rff_tol(W, b, theta, ic.RFF_BIAS, Z)
        assert np.all(tol.max(axis=1) <= ic.rff_tol_cap(theta, ic.RFF_BIAS)), (n, d, S, tol.max())
        ref = ic.rff_reference(W, b, theta, ic.RFF_BIAS, Z)
        muts = ic.rff_mutations(W, b, theta, ic.RFF_BIAS, Z)
        assert len(muts) == (4 if n > 1 else 2), (n, sorted(muts))
        for name, v in muts.items():
            ratio = np.abs((v - ref).astype(float)) / tol
            for s in range(S):                                            # in every draw, at more than one candidate
                assert np.sum(ratio[s] >= 100.0) > 1, (name, n, d, S, s, np.sort(ratio[s])[-2:])
                weakest = min(weakest, float(np.sort(ratio[s])[-2]))
    print('d = %d: the weakest mutation still misses by %.3g tolerances at its second-worst candidate' % (d, weakest))
