"""The kernel families whose launcher picks a template case from a run-time size: the selection rules restated in Python, the
case lists of tests/test_gpu_instantiations.py (and of the bound tests' second parametrisation), and the inputs, the long-double
reference and the tolerance of the Thompson cases.  Shared by tests/test_instantiation_cases_cpu.py, which holds the lists against the
instantiations the built library contains, and by the GPU tests, which run them.

  k_rff_mfma5<JF, NSUB, DB>       launch_rff_mfma (kernels_rff.hip)        rff5_case(n, d)
  k_path_update<KID, NJB>         launch_path_update (kernels_path.hip)    path_cases(kernel, S)
  k_tri_matvec_rb<MBT, 4>         predict_grad_enqueue (kernels_grad.hip)  tri_rb_cases(d, M, form, kern)
  k_bound_mfma<KS, NC>            launch_bound_mfma (kernels_sweep.hip)    bound_case(d)
  k_bound_mfma32<KS, NC, false>   launch_bound_mfma32 (kernels_bound32.hip)    "
"""
import re
import shutil
import subprocess

import numpy as np

import devmath_ref as dm

# ---------------------------------------------------------------------------------------------------------------------
# the instantiations a library holds
# ---------------------------------------------------------------------------------------------------------------------
_STUB = re.compile(r'__device_stub__(\w+?)(?:<([^()]*)>)?\(')


def _symbol_tool():
    """llvm-nm where the toolchain ships it, binutils' nm or the toolchain's llvm-readelf otherwise: (argv prefix)."""
    import glob
    import os
    dirs = [os.path.dirname(p) for p in glob.glob('/opt/rocm*/lib/llvm/bin/clang')] + [os.path.dirname(p) for p in glob.glob('/opt/rocm*/llvm/bin/clang')]
    for name, args in (('llvm-nm', ['-C']), ('nm', ['-C']), ('llvm-readelf', ['-s', '-W', '-C'])):
        exe = shutil.which(name) or next((os.path.join(d, name) for d in dirs if os.path.exists(os.path.join(d, name))), None)
        if exe:
            return [exe] + args
    raise RuntimeError('no llvm-nm, nm or llvm-readelf to list the library\'s symbols with')


def kernel_instantiations(lib_path):
    """{kernel name: set of template-argument tuples (strings; () for a plain kernel)} from the host stubs of lib_path."""
    out = subprocess.run(_symbol_tool() + [lib_path], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    found = {}
    for name, targs in _STUB.findall(out):
        args = tuple(a.strip() for a in targs.split(',')) if targs else ()
        found.setdefault(name, set()).add(args)
    return found


# ---------------------------------------------------------------------------------------------------------------------
# the selection rules
# ---------------------------------------------------------------------------------------------------------------------
def rff5_case(n, d):
    """(JF, NSUB, DB) of launch_rff_mfma, None where another kernel runs (n > 128: several feature tiles; dp > 32)."""
    dp = (d + 3) // 4 * 4
    if n > 128 or dp > 32:
        return None
    rem = n & 15
    if rem == 0 or rem > 8:
        jf, nsub = (n + 15) // 16, 0
    else:
        jf, nsub = n // 16, (rem + 3) // 4
    return jf, nsub, dp <= 16


def path_njb(S):
    """NJB of every group of 64 draws of launch_path_update, in launch order."""
    return [(min(64, S - 64 * g) + 15) // 16 for g in range((S + 63) // 64)]


KIDS = {'se': 0, 'matern5': 1, 'matern3': 2, 'matern1': 3}


def path_cases(kernel, S):
    return {(KIDS[kernel], njb) for njb in path_njb(S)}


GB = 16                                   # right-hand sides of one pass of predict-with-gradients (ws_layout.h)


def tri_rb_cases(d, M, form, kern):
    """(MBT, mode) of every k_tri_matvec_rb launch of one gpx_predict call with gradients at M points (options grad_form, grad_kernel);
    mode 0: the pass over T, 1: over U.  Empty where k_tri_matvec_multi runs instead."""
    one_pass = 1 + d <= GB and form != 1 and (form == 2 or M == 1)
    chunk = GB // (1 + d) if one_pass else GB
    out = set()
    for m0 in range(0, M, chunk):
        mb = min(chunk, M - m0)
        if one_pass:
            out.add((mb * (1 + d), 0))
        elif kern == 1 or (kern < 0 and M > 1):
            out |= {(mb, 0), (mb, 1)}
    return out


def bound_case(d):
    """(KS, NC) of launch_bound_mfma / launch_bound_mfma32 for the SE covariance, d <= 18."""
    nc = (d + 3) // 4 < (d + 5) // 4
    return ((d + 3) // 4 if nc else (d + 5) // 4), nc


# ---------------------------------------------------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------------------------------------------------
RFF_DS = (3, 9, 16, 17, 32)               # dp = 4, 12, 16, 20, 32: 1, 3, 4, 5, 8 k-groups; 16 | 17 the DB boundary; 32 raises the LDS limit
RFF_NS = tuple(range(1, 129))
RFF_S, RFF_S1_NS = 3, (8, 24, 100)        # three draws everywhere: both LDS images and the last tile; one draw at three n
RFF_M, RFF_BIAS, RFF_W_SCALE, RFF_K = 300, 0.25, 2.0, 10


def rff_cases(d):
    """(n, S) of the Thompson test at input dimension d."""
    return [(n, RFF_S) for n in RFF_NS] + [(n, 1) for n in RFF_S1_NS]


PATH_CASES = ('n129_d20', 'n300_d3')      # keys of tests/test_gpu_path.py CASES
PATH_SS = (17, 33, 48, 81)                # NJB 2, 3, 3 and (4, 2)
PATH_N = 100
PATH_SS_BEFORE = (1, 2, 3, 5, 65)         # what tests/test_gpu_path.py sweeps: NJB 1 and (4, 1)
PATH_ALONE = {48: (16, 32, 47), 81: (80,)}    # draws swept alone: the bits they have in the full call

GRAD_N, GRAD_KERNELS, GRAD_CS = 300, ('se', 'matern3'), (128, 0)      # Np = 384: three segments of 128 columns, the last partial; 0 = default
GRAD_SINGLE_DS = tuple(range(1, 16))      # single points, one pass: MBT = 1 + d
GRAD_TWO_PASS_D, GRAD_TWO_PASS_MB = 3, tuple(range(1, 17))            # grad_form = 1, grad_kernel = 1: MBT = mb on T and on U
GRAD_ONE_PASS_DS = (1, 2, 3)              # grad_form = 2, batches of 1 .. 16 // (1 + d) points: MBT = mb (1 + d)


def grad_calls():
    """(d, M, grad_form, grad_kernel) of every predict-with-gradients call shape of the gradient tests."""
    calls = [(d, 1, 0, -1) for d in GRAD_SINGLE_DS]
    calls += [(GRAD_TWO_PASS_D, mb, 1, 1) for mb in GRAD_TWO_PASS_MB]
    calls += [(d, M, 2, -1) for d in GRAD_ONE_PASS_DS for M in range(1, GB // (1 + d) + 1)]
    return calls


BOUND_DS_BEFORE = (1, 2, 8, 9, 16)        # tests/test_gpu_prune_bound_mfma.py DS
BOUND_DS = (3, 4, 5, 6, 11, 12, 13, 14, 17, 18)
BOUND_NS = (130, 1024)


# ---------------------------------------------------------------------------------------------------------------------
# the Thompson cases: inputs, reference, tolerance, mutations
# ---------------------------------------------------------------------------------------------------------------------
def rff_candidates(d):
    """M = 300 candidates in [-1, 1]^d: two full tiles of 128 and a partial one."""
    return np.random.RandomState(900 + d).rand(RFF_M, d) * 2.0 - 1.0


def rff_draws(n, d, S):
    """W (S, n, d) = 2 N(0, 1), b (S, n) in [0, 2 pi), theta_j = +-(0.05 + 0.1 j / n): all magnitudes different, so no two features can
    change places unnoticed.  The scale of W keeps the tolerance below 1e-12 max(1, sum |theta| + |bias|) up to d = 32."""
    rng = np.random.RandomState(100000 * S + 1000 * d + n)
    W = rng.randn(S, n, d) * RFF_W_SCALE
    b = rng.rand(S, n) * 2.0 * np.pi
    sign = np.where(rng.rand(S, n) < 0.5, -1.0, 1.0)
    theta = sign * (0.05 + 0.1 * np.arange(n) / n)[None, :]
    return W, b, theta


def rff_terms(W, b, theta, Z):
    """theta_j cos(w_j . z + b_j) per (draw, candidate, feature) in numpy.longdouble (64-bit mantissa: 2^-11 of a double's ulp)."""
    L = np.longdouble
    z = np.matmul(Z.astype(L)[None, :, :], np.transpose(W.astype(L), (0, 2, 1))) + b.astype(L)[:, None, :]
    return theta.astype(L)[:, None, :] * np.cos(z)


def rff_value(terms, bias):
    return np.longdouble(bias) + terms.sum(axis=2)


def rff_reference(W, b, theta, bias, Z):
    """bias + sum_j theta_j cos(w_j . z + b_j), (S, M), long double."""
    return rff_value(rff_terms(W, b, theta, Z), bias)


def rff_tol(W, b, theta, bias, Z):
    """The bound of test_thompson_value_of_both_cosines_agrees_on_a_realistic_draw (tests/test_gpu_devmath.py), one-sided because the
    reference is exact: per feature the projection's gamma_{d+1} (|b_j| + sum |w z|), which the cosine passes on 1:1, cos_cw's
    COS_POLY_ABS + |n_j| C3 and 2 u for the product and the rounded theta-weighted term; gamma_n sum |theta| for the sum over the
    features in any order; 2 u |bias|.  (S, M)."""
    S, n, d = W.shape
    gam = lambda m: m * dm.U / (1 - m * dm.U)
    tol = np.empty((S, len(Z)))
    for s in range(S):
        proj = np.abs(Z) @ np.abs(W[s]).T + np.abs(b[s])                  # (M, n)
        zz = Z @ W[s].T + b[s]
        per = gam(d + 1) * proj + dm.COS_POLY_ABS + np.abs(dm.cos_cw_n(zz)) * dm.C3 + 2 * dm.U
        tol[s] = per @ np.abs(theta[s]) + gam(n) * np.abs(theta[s]).sum() + 2 * dm.U * abs(bias)
    return tol


def rff_tol_cap(theta, bias):
    """What test_random_thompson_shapes_against_numpy grants, per draw: 1e-12 max(1, sum |theta| + |bias|)."""
    return 1e-12 * np.maximum(1.0, np.abs(theta).sum(axis=1) + abs(bias))


def rff_b_swap_columns(n, d):
    """The column 16 JF -- the first one of the remainder sub-tiles -- and its neighbour; where the case has no remainder columns
    (NSUB = 0), the first column of its last 16-column group.  None at n = 1."""
    if n == 1:
        return None
    jf = rff5_case(n, d)[0]
    c = 16 * jf if 16 * jf < n else 16 * (jf - 1)
    return c, (c + 1 if c + 1 < n else c - 1)


RFF_ROWS_EXCHANGED = (1, 5)               # one lane group of four rows apart: register index r against lane index fk of the accumulator


def rff_mutations(W, b, theta, bias, Z):
    """{name: values (S, M)} of the reference recomputed with one defect each.  At n = 1 the two that need a second feature are absent."""
    S, n, d = W.shape
    terms = rff_terms(W, b, theta, Z)
    out = {'last feature dropped': rff_value(terms[:, :, :n - 1], bias)}
    if n > 1:
        t2 = theta.copy()
        t2[:, [n - 2, n - 1]] = theta[:, [n - 1, n - 2]]
        m = terms.copy()
        m[:, :, n - 2:] = rff_terms(W[:, n - 2:], b[:, n - 2:], t2[:, n - 2:], Z)
        out['theta of the last two features swapped'] = rff_value(m, bias)
        c, c2 = rff_b_swap_columns(n, d)
        cols = [c, c2]
        m = terms.copy()
        m[:, :, cols] = rff_terms(W[:, cols], b[:, cols[::-1]], theta[:, cols], Z)
        out['b of column 16 JF swapped with its neighbour'] = rff_value(m, bias)
    v = rff_value(terms, bias).copy()
    i, j = RFF_ROWS_EXCHANGED
    v[:, [i, j]] = v[:, [j, i]]
    out['two candidate rows exchanged'] = v
    return out
