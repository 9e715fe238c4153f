"""The fp32 bound kernel's sign-homogeneous row tiles and factorised exponent (pybo_amd/csrc/bound_f32.h) on the host.

tests/c/bound_f32_fact_check.cpp includes the header k_bound_mfma32, k_bound_aug and k_bound_guard include and runs the kernel's
arithmetic in float (-ffp-contract=off; exp2f stands in for v_exp_f32): the scaled weights w' = fl32(w r_i), the rows reordered by sign
with the extra zero tile, per-lane sums P and Nn of depth Np / 16, A = P + Nn and B = P - Nn, the column factor, bound32_hi.  For
d in {1, 2, 8, 9, 16} at Np = 1024 it walks random weights, all positive, all negative (N = Np), exactly 16 m positives with no zero
row but the extra tile's (N = Np), one positive, alternating signs, zero weights among the live rows, a weight that is normal in fp32
while its w' is not (the factorised walk's guard must refuse, the fp32 kernel's must not), L R_x R_z just inside and just outside that
guard, and a candidate on an observation; every case in both forms wherever the form's margin is finite.  For every candidate

    dot_hi >= the long-double dot          and          dot_hi - dot <= 2 E sum |w_i| k_i + 3 F

with the E and F of bound_f32.h unchanged; the tiles before tpos hold no negative and the others no positive weight; no lane's sum
has more than Np / 16 FMAs with a non-zero weight; behind the guard no k' leaves fp32's normal range.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import subprocess

from test_bound_exp_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'bound_f32_fact_check.cpp')
DS = (1, 2, 8, 9, 16)
KINDS = ('random', 'all positive', 'all negative', '16 m positives', 'one positive', 'alternating', 'zero weights', "subnormal w'",
         'range inside', 'range outside', 'on an observation')
CASES = len(DS) * len(KINDS)


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
    assert lines[-1] == 'bound f32 fact ok %d cases' % CASES and len(lines) == CASES + 1, lines
    return lines[:-1]


def test_the_margin_covers_both_walks_on_every_sign_pattern_and_the_guard_refuses_what_it_must(tmp_path):
    lines = _run(_build(tmp_path, 'bound_f32_fact_check', ['-O2']))
    for d in DS:
        for kind in KINDS:
            ln = [x for x in lines if x.startswith('%s d=%d ' % (kind, d))]
            assert len(ln) == 1, (kind, d)
            ln = ln[0]
            fact = ' fact    ' in ln
            assert fact == (kind not in ("subnormal w'", 'range outside')), ln
            assert (' fp32 ' in ln) == (not kind.startswith('range')), ln
            e = float(ln.split(' E ')[1].split()[0])
            assert 0.0 < e <= 2.0 ** -10, ln
            x = float(ln.split('L Rx Rz')[1].split()[0])
            if kind == 'range inside':
                assert 119.0 < x <= 120.0 / (1.0 + 2.0 ** -10), ln
            if kind == 'range outside':
                assert 120.0 < x < 121.0, ln
            tpos = int(ln.split(' tpos ')[1].split()[0])
            if kind == 'all positive':
                assert tpos == 63, ln                      # 1000 positives: 62.5 tiles
            if kind == 'all negative':
                assert tpos == 0, ln
            if kind == '16 m positives':
                assert tpos == 23, ln
            if kind == 'one positive':
                assert tpos == 1, ln
            plain, factv = float(ln.split('<=')[1].split()[0]), float(ln.split('plain,')[1].split()[0])
            assert 0.0 < plain < 1.0 and (0.0 < factv < 1.0 if fact else factv == 0.0), ln


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'bound_f32_fact_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_kernels_call_the_header_the_check_includes():
    """One definition of the row order, the norm factor and the factorised walk's guards: k_bound_aug, k_bound_guard, k_bound_mfma32
    and the host program call bound_f32.h."""
    csrc = os.path.join(ROOT, 'pybo_amd', 'csrc')
    kern = open(os.path.join(csrc, 'kernels_bound32.hip')).read()
    sweep = open(os.path.join(csrc, 'kernels_sweep.hip')).read()
    aug = sweep[sweep.index('void k_bound_aug('):sweep.index('void k_bound_rz(')]
    for fn in ('bound32_row_dest(', 'bound32_tpos(', 'bound32_norm_factor(', 'bound32_bad_weight_fact('):
        assert fn in aug, fn
    guard = sweep[sweep.index('void k_bound_guard('):sweep.index('void k_bound_mfma(')]
    assert 'bound32_fact_ok(' in guard
    assert 'bound32_norm_factor(' in kern and 'BM_SC_TPOS32' in kern and 'BM_SC_FACT32' in kern
    src = open(SRC).read()
    assert '#include "../../pybo_amd/csrc/bound_f32.h"' in src
    for fn in ('bound32_row_dest(', 'bound32_tpos(', 'bound32_norm_factor(', 'bound32_bad_weight_fact(', 'bound32_fact_ok(', 'bound32_hi('):
        assert fn in src, fn
