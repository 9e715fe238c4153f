"""The constraint fold of a constrained sweep (pybo_amd/csrc/acq_core.h: con_fold) on the host, bit for bit against numpy.

tests/c/con_fold_check.cpp is a stand-alone program around the header k_con_fold includes.  Without arguments it prints con_fold over
every pair of a set of special values (0, -0, denormals, huge values, 1, its neighbours, +inf, NaN); given a file of rows
(v_0, p_1 .. p_J) it writes v_J.  Here: the printed lines against numpy's v * min(p, 1); 200 000 drawn pairs bit for bit and
con_fold(v, p) <= v for every v >= 0, p in [0, 1]; NaN in, NaN out; and the one new step of the pruning argument (DESIGN.md section
2.3) -- a bound on v_0 is a bound on v_J after any chain of factors.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import con_ref
from test_ens_prune_cpu import _special

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'con_fold_check.cpp')


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/con_fold_check.cpp with')


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe, *args):
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'con fold ok', lines[-3:]
    return [ln.split() for ln in lines[:-1]]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('con_fold'), 'con_fold_check', ['-O2'])


def _fold_rows(exe, tmp_path, rows):
    """v_J of every row (v_0, p_1 .. p_J), by the compiled con_fold."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    rows.tofile(src)
    out = _run(exe, src, dst, str(rows.shape[1] - 1))
    assert out[-1] == ['rows', str(len(rows))]
    return np.fromfile(dst, dtype=np.float64)


def _same_bits(a, b):
    """bit for bit; any NaN equals any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def test_special_values_agree_with_numpy_bit_for_bit(exe):
    lines = [f for f in _run(exe) if f[0] == 'fold']
    assert len(lines) == 15 * 15
    seen_v, seen_p = set(), set()
    for _, v, p, r in lines:
        v, p, r = float.fromhex(v), float.fromhex(p), float.fromhex(r)
        with np.errstate(invalid='ignore'):
            want = np.float64(v) * np.minimum(np.float64(p), 1.0)
        assert (math.isnan(r) and math.isnan(want)) or struct.pack('<d', r) == struct.pack('<d', float(want)), (v, p, r, want)
        if math.isnan(v) or math.isnan(p):
            assert math.isnan(r)
        seen_v.add(v), seen_p.add(p)
    for need in (0.0, 5e-324, 1.0, np.nextafter(1.0, 2.0), np.inf, 1e300):
        assert need in seen_v and need in seen_p, need


def test_a_factor_never_raises_a_non_negative_value(exe, tmp_path):
    rng = np.random.RandomState(7)
    m = 200000
    v = _special(rng, m)
    # p in [0, 1]: uniform, the ends themselves, numbers just below 1 and tiny ones
    p = rng.rand(m)
    how = rng.randint(0, 8, size=m)
    p[how == 0] = 0.0
    p[how == 1] = 1.0
    p[how == 2] = np.nextafter(1.0, 0.0)
    p[how == 3] = np.exp(rng.uniform(-740.0, 0.0, size=m))[how == 3]
    got = _fold_rows(exe, tmp_path, np.column_stack([v, p]))
    with np.errstate(invalid='ignore'):
        assert _same_bits(got, v * np.minimum(p, 1.0)) and _same_bits(got, con_ref.fold(v, p))
    ok = ~np.isnan(got)                          # (inf * 0)
    assert np.array_equal(~ok, np.isinf(v) & (p == 0.0))
    assert np.all(got[ok] <= v[ok]) and np.all(got[ok] >= 0.0)
    # a factor above 1 is clamped to 1: the value itself comes back
    above = _fold_rows(exe, tmp_path, np.column_stack([v, 1.0 + rng.rand(m) * np.exp(rng.uniform(-36.0, 700.0, size=m))]))
    assert _same_bits(above, v)


def test_nan_in_either_argument_gives_nan(exe, tmp_path):
    rng = np.random.RandomState(8)
    v, p = _special(rng, 1000), rng.rand(1000)
    rows = np.vstack([np.column_stack([np.full(1000, np.nan), p]), np.column_stack([v, np.full(1000, np.nan)])])
    assert np.isnan(_fold_rows(exe, tmp_path, rows)).all()


@pytest.mark.parametrize('J', [1, 2, 3, 16])
def test_a_bound_on_the_objective_s_value_bounds_the_product(exe, tmp_path, J):
    rng = np.random.RandomState(10 + J)
    m = 200000
    a = _special(rng, m)
    how = rng.randint(0, 5, size=m)
    with np.errstate(over='ignore', invalid='ignore'):
        ub = np.select([how == 0, how == 1, how == 2, how == 3], [a, np.nextafter(a, np.inf), a * (1.0 + 1e-6), a + 1e-9], np.inf)
    P = rng.rand(m, J)
    edge = rng.randint(0, 6, size=(m, J))
    P[edge == 0] = 1.0
    P[edge == 1] = 0.0
    P[edge == 2] = 1.0 + rng.rand(m, J)[edge == 2]          # what only a device erfc out of range could return: clamped
    nan = rng.rand(m) < 0.01
    P[nan, rng.randint(0, J, size=m)[nan]] = np.nan
    assert np.all(ub >= a)
    v = _fold_rows(exe, tmp_path, np.column_stack([a, P]))
    assert _same_bits(v, con_ref.chain(a, list(P.T)))
    assert np.all(np.isnan(v[nan]))                          # a NaN anywhere makes v_J NaN: it ranks last
    fin = ~np.isnan(v)
    assert np.all(ub[fin] >= v[fin])


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path, 'con_fold_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    _run(san)
    rows = np.column_stack([np.linspace(0.0, 2.0, 64), np.linspace(0.0, 1.5, 64), np.linspace(1.0, 0.0, 64)])
    assert len(_fold_rows(san, tmp_path, rows)) == 64


def test_the_kernel_calls_the_function_the_check_includes():
    import re
    assert '#include "../../pybo_amd/csrc/acq_core.h"' in open(SRC).read()
    ens = open(os.path.join(CSRC, 'kernels_ens.hip')).read()
    assert '#include "acq_core.h"' in ens and 'k_con_fold' in ens and ens.index('fp contract(off)') < ens.index('k_con_fold')
    body = ens[ens.index('void k_con_fold'):ens.index('static inline int ew_blocks')]
    assert body.count('= con_fold(') == 2 and ' * p' not in body and '*=' not in body          # the products are con_fold's, not the kernel's
    everything = '\n'.join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h')))
    assert len(re.findall(r'^GPX_ACQ_FN[^\n(]*\bcon_fold\(', everything, flags=re.M)) == 1
