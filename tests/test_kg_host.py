"""The knowledge gradient's line mathematics (pybo_amd/csrc/kg_math.h) on the host, against the 50-digit truth of tests/kg_ref.py.

tests/c/kg_math_check.cpp is a stand-alone program around the header the kernels of kernels_kg.hip include: it runs kg_value /
kg_weights over designed and random line sets with n = 1, 2, 3, 64, 128 (all slopes equal, all intercepts equal, duplicated lines,
three nearly concurrent lines, slopes of 1e-300, crossings beyond |c| = 38 and around the switches at 8 and 39), checks what it can
check alone (finite, >= 0, sum P_j = 1, sum w_j = 0, accessor independence) and prints every set with its value in hexadecimal.
Here every printed value is held against kg_truth AT THE DOUBLES PRINTED within kg_bound, the bound the header derives -- not a
measured number with padding.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'kg_math_check.cpp')
TAGS = {'random', 'equal_slopes', 'equal_intercepts', 'duplicates', 'concurrent', 'tiny_slopes', 'tiny_slopes_far', 'far_crossings',
        'switch_8', 'cut_39'}


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/kg_math_check.cpp with')


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'kg math ok', lines[-3:]
    sets = []
    for ln in lines[:-2]:
        f = ln.split()
        assert f[0] == 'set', ln
        n = int(f[2])
        vals = [float.fromhex(x) for x in f[3:]]
        assert len(vals) == 1 + 2 * n
        sets.append((f[1], vals[0], np.array(vals[1::2]), np.array(vals[2::2])))
    assert lines[-2] == 'sets %d' % len(sets)
    return sets


def test_every_value_is_within_the_derived_bound_of_the_truth(tmp_path):
    sets = _run(_build(tmp_path, 'kg_math_check', ['-O2']))
    assert {t for t, _, _, _ in sets} == TAGS and sorted({len(a) for _, _, a, _ in sets}) == [1, 2, 3, 64, 128]
    worst = 0.0
    for tag, got, a, b in sets:
        want, bound = kg_ref.kg_truth(a, b), kg_ref.kg_bound(a, b)
        err = abs(got - want)
        assert err <= bound, (tag, len(a), got, want, err, bound)
        if bound > 0.0:
            worst = max(worst, err / bound)
        # the bound is tight enough to pin something: 100 times under the 1e-6 parity tolerance it feeds, relative to the slopes' spread
        assert bound <= 1e-8 * max(np.max(np.abs(b - b[0])), 1e-300) + 128 * 2.0 ** -1022
        if tag == 'equal_slopes' or len(a) == 1:
            assert got == 0.0
        if tag == 'equal_intercepts':
            assert abs(got - (b.max() - b.min()) * 0.39894228040143267794) <= bound
    print('worst error / bound over %d sets: %.3g' % (len(sets), worst))
    # the designed sets reach what they were designed for
    far = [(a, b) for t, _, a, b in sets if t == 'far_crossings' and len(a) > 1]
    assert far and all(min(abs(float(lo)) for _, lo, _ in kg_ref.envelope(a, b)[1:]) > 38.0 for a, b in far)


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'kg_math_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_kernels_include_the_header_the_check_includes():
    ksrc = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'kernels_kg.hip')).read()
    assert '#include "kg_math.h"' in ksrc and 'kg_partial(' in ksrc and 'kg_combine(' in ksrc and 'kg_weights(' in ksrc
    assert '#include "../../pybo_amd/csrc/kg_math.h"' in open(SRC).read()
    hdr = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'kg_math.h')).read()
    assert 'threadIdx' not in hdr and 'hip_runtime' not in hdr          # plain C++: no HIP type
    build = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'build.sh')).read()
    assert 'kg_math.h' in build and 'kernels_kg' in build                # a dependency of the incremental build, a translation unit
