"""The table-driven exponential of the bound pass's matrix-pipe kernel (pybo_amd/csrc/bound_exp.h) on the host, bit for bit the device's.

The header is plain C++ with explicit fma and no contraction, so every operation rounds once on either side;
tests/c/bound_exp_check.cpp includes the header k_bound_mfma includes and holds, over 3.0e6 arguments (uniform in [-60, 0] and in
[-746, 0], 10^4 in [-1e-3, 0], every grid point k ln2 / 128 -1, 0, +1 ulp for |k| <= 512, 0, -0.0, -745.2, -746, -1e9, -inf, NaN):

  table       T[j] == 2^(j / 128) rounded from long double;
  accuracy    <= 1.05 ulp against long double expl wherever the result is >= 2^-1022 (measured: 0.9971 ulp, printed);
  values      exactly 1.0 at +-0, +0.0 at -inf, -1e9, -746 and below, NaN at NaN (the kernel's own variant, whose floor is a
              one-instruction maximum, returns the floor's 0 for a NaN: the kernel restores a candidate's NaN per column);
  variants    the compare-and-select floor and the maximum agree bit for bit on every argument that is not NaN;
  monotone    non-decreasing over the sorted sample.

Printed, not part of the sorted sample: the seams of j, (k - 1/2) ln2 / 128 -1, 0, +1 ulp.  The two sides of a seam take two
table entries, each rounded on its own, and neighbouring doubles across a seam can come out one ulp in the wrong order (13 of the
513 seams down to -4 ln2); never more than one ulp, and the accuracy bound holds there as everywhere.  EI's monotonicity argument
 is about the exact function and charges the evaluation's error to eps_k.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'bound_exp_check.cpp')
ULP_BOUND = 1.05


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/bound_exp_check.cpp with')


def build_checker(directory, name='bound_exp_check', flags=('-O2',)):
    """The checker as an executable in `directory` (tests/test_gpu_bound_exp.py feeds it the device's arguments)."""
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off']
                          + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'bound exp ok' and len(lines) == 4, lines
    nargs = int(lines[0].split()[1])
    worst = float(lines[1].split()[2])
    nonmono = int(lines[2].split()[2])
    assert nargs >= 3000000
    assert worst <= ULP_BOUND, worst
    assert nonmono == 0
    return worst


def test_the_exponential_meets_its_bound_and_its_special_values(tmp_path):
    worst = _run(build_checker(tmp_path))
    assert worst > 0.5                       # a figure below half an ulp would be a broken measure, not a better function


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(build_checker(tmp_path, 'bound_exp_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_kernel_includes_the_header_the_check_includes():
    """One definition: kernels_sweep.hip and the host program include bound_exp.h; the kernel calls it and not exp_nonpos."""
    ksrc = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'kernels_sweep.hip')).read()
    assert '#include "bound_exp.h"' in ksrc and 'double bound_exp(' not in ksrc
    body = ksrc[ksrc.index('void k_bound_mfma('):ksrc.index('void launch_bound_mfma(')]
    assert 'bound_exp<false>(' in body and 'exp_nonpos(' not in body
    assert '#include "../../pybo_amd/csrc/bound_exp.h"' in open(SRC).read()
    hdr = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'bound_exp.h')).read()
    assert '#include' not in hdr and 'threadIdx' not in hdr      # plain C++: no header, no HIP type
    assert 'bound_exp.h' in open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'build.sh')).read()      # a dependency of the incremental build
