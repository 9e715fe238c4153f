"""The error margin of the bound pass's fp32 matrix-pipe kernel (pybo_amd/csrc/bound_f32.h) on the host.

tests/c/bound_f32_check.cpp includes the header k_bound_mfma32 and k_bound_guard include and runs the kernel's arithmetic in float
(-ffp-contract=off; exp2f stands in for v_exp_f32, whose error term stays in the margin) on `_problem`-style inputs for
d in {1, 2, 8, 9, 16} and on the adversarial cases: a candidate on an observation, weights of alternating sign spanning 1e30, a weight
that is subnormal in fp32 and one beyond its range (the guard must refuse both), exponents beyond -87 inside the guard (covariances
that come back as 0), and candidates so far that the guard declines.  For every candidate it asserts

    dot_hi >= the long-double dot          and          dot_hi - dot <= 2 E sum |w_i| k_i + 3 F

(F, the flush term, can be lost once and is added once).  The program prints, per case, how much of the margin was used: the lower
figure must stay positive, the upper one below 1; on smooth inputs the rounding errors cancel and both sit near E B itself.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import subprocess

from test_bound_exp_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'bound_f32_check.cpp')
CASES = 11


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags)
                          + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'bound f32 ok %d cases' % CASES and len(lines) == CASES + 1, lines
    return lines[:-1]


def test_the_margin_covers_the_float_arithmetic_on_problems_and_adversarial_inputs(tmp_path):
    lines = _run(_build(tmp_path, 'bound_f32_check', ['-O2']))
    used = [ln for ln in lines if ' fp32 ' in ln]
    refused = [ln for ln in lines if ' refused ' in ln]
    assert len(used) == 8 and len(refused) == 3, lines
    assert all(name in ' '.join(refused) for name in ('subnormal weight', 'overflowing weight', 'far candidates'))
    assert any('exponents beyond -87' in ln and 'flushed entries' in ln for ln in used)
    for ln in used:
        e = float(ln.split(' E ')[1].split()[0])
        assert 0.0 < e <= 2.0 ** -10, ln


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'bound_f32_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_kernel_and_the_guard_include_the_header_the_check_includes():
    """One definition of E, the factor, the flush term and dot_hi: the kernel, the guard and the host program call bound_f32.h."""
    csrc = os.path.join(ROOT, 'pybo_amd', 'csrc')
    kern = open(os.path.join(csrc, 'kernels_bound32.hip')).read()
    sweep = open(os.path.join(csrc, 'kernels_sweep.hip')).read()
    assert '#include "bound_f32.h"' in kern and 'bound32_hi(' in kern
    assert '#include "bound_f32.h"' in sweep
    guard = sweep[sweep.index('void k_bound_guard('):sweep.index('void k_bound_mfma(')]
    for fn in ('bound32_E(', 'bound32_factor(', 'bound32_flush('):
        assert fn in guard, fn
    assert 'bound32_bad_weight(' in sweep
    assert '#include "../../pybo_amd/csrc/bound_f32.h"' in open(SRC).read()
    hdr = open(os.path.join(csrc, 'bound_f32.h')).read()
    assert 'threadIdx' not in hdr and 'hip_runtime' not in hdr                      # plain C++
    build = open(os.path.join(csrc, 'build.sh')).read()
    assert 'bound_f32.h' in build                                                     # a dependency of the incremental build
    assert 'kernels_bound32.hip -fno-slp-vectorize' in build                          # (why: the file's header)
