"""The fantasised picks' per-candidate arithmetic (pybo_amd/csrc/acq_core.h: fant_mean_step, fant_fold / fant_average, fant_incumbent) on
the host, bit for bit against numpy.

tests/c/fant_core_check.cpp is a stand-alone program around the header kernels_batch.hip includes.  It checks every result against
long-double arithmetic and against the zero-innovation identity itself (zero innovations leave the believer's mean, S = 1 the value's own
bits) and prints inputs and results in hexadecimal; here every line is recomputed FROM THE DOUBLES PRINTED by the expression the library
promises -- one rounded product and one rounded addition per row of V in pick order, the fantasies summed in order from the first and
divided once, the incumbent's last coefficient s2 / d -- and compared bit for bit.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_acq_core_host import _compiler, _f, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'fant_core_check.cpp')


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'fant core ok', lines[-3:]
    return [ln.split() for ln in lines[:-1]]


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp('fant_core'), 'fant_core_check', ['-O2']))


def _walk(m, v, e):
    m = np.float64(m)
    for a, b in zip(v, e):
        prod = np.float64(a) * np.float64(b)
        m = m + prod
    return m


def test_the_mean_walk_rounds_every_product_in_pick_order(lines):
    lengths, zero = set(), 0
    for f in (f for f in lines if f[0] == 'mean'):
        j = int(f[1])
        w = _f(f[2:])
        mu, v, e, m = w[0], w[1:1 + j], w[1 + j:1 + 2 * j], w[1 + 2 * j]
        assert len(w) == 2 + 2 * j
        assert _same(m, _walk(mu, v, e)), f
        if j and not np.any(e):
            assert _same(m, mu), f                                   # the believer's mean, bit for bit
            zero += 1
        lengths.add(j)
    assert {0, 1, 3, 5, 63} <= lengths and zero >= 10


def test_the_average_sums_in_fantasy_order_and_divides_once(lines):
    sizes = set()
    for f in (f for f in lines if f[0] == 'avg'):
        S = int(f[1])
        w = _f(f[2:])
        vals, value = w[:S], w[S]
        acc = np.float64(vals[0])
        for x in vals[1:]:
            acc = acc + np.float64(x)
        assert _same(value, acc / np.float64(S)), f
        if not np.any(np.isnan(vals)):
            assert _same(value, np.mean(np.stack([vals, vals], axis=1), axis=0)[0]), f      # numpy's mean over axis 0
        if S == 1:
            assert _same(value, vals[0])
        sizes.add(S)
    assert {1, 2, 3, 5, 16, 64} <= sizes


def test_the_incumbent_is_the_mean_at_the_pick_after_its_own_observation(lines):
    seen, raised, kept = set(), 0, 0
    for f in (f for f in lines if f[0] == 'inc'):
        j, cs, es = int(f[1]), int(f[2]), int(f[3])
        w = _f(f[4:])
        t, mu, s2, d = w[:4]
        cross, eps, r = w[4:4 + j], w[4 + j:5 + 2 * j], w[5 + 2 * j]
        assert len(w) == 6 + 2 * j
        u = _walk(_walk(mu, cross, eps[:j]), [np.float64(s2) / np.float64(d)], eps[j:])
        with np.errstate(invalid='ignore'):
            want = np.fmax(np.float64(t), u)                         # fmax: a NaN u leaves t
        assert _same(r, want), f
        raised += int(r > t)
        kept += int(r == t)
        seen.add((j, cs, es))
    assert {(3, 1, 1), (3, 5, 3), (3, 1, 64), (0, 1, 1), (1, 1, 1)} <= seen and raised >= 3 and kept >= 4


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'fant_core_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_kernels_use_the_header_the_check_includes():
    assert '#include "../../pybo_amd/csrc/acq_core.h"' in open(SRC).read()
    src = open(os.path.join(CSRC, 'kernels_batch.hip')).read()
    assert '#include "acq_core_dev.h"' in src
    for fn in ('fant_mean_step', 'fant_fold', 'fant_average', 'fant_incumbent'):
        assert re.search(r'\b%s\(' % fn, src), fn
    everything = '\n'.join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h', '.cpp')))
    for fn in ('fant_mean_step', 'fant_fold', 'fant_average', 'fant_incumbent'):
        assert len(re.findall(r'^(?:GPX_ACQ_FN|__device__ __forceinline__)[^\n(]*\b%s\(' % fn, everything, flags=re.M)) == 1, fn
    # the device scores with the believer's own fold and moments: one recurrence, two values.  Both scoring kernels are the frame around
    # batch_cand (the fold and the moments, stated once in acq_core.h), both pick kernels are single_pick (the merge, the member's part
    # with its scalars, the gather), and no kernel of the file restates any of it
    def body(name):
        m = re.search(r'void %s\(.*?\n}\n' % re.escape(name), src, flags=re.S)
        assert m, name
        return m.group(0)
    for kernel in ('k_batch_score', 'k_fant_score'):
        assert 'batch_score_frame(' in body(kernel) and 'batch_cand(j, M, n, e, s2_out)' in body(kernel), kernel
    for kernel in ('k_batch_pick', 'k_fant_pick'):
        assert 'single_pick(' in body(kernel), kernel
    for fn in ('merge_pick', 'pick_member', 'pick_gather'):
        assert '%s(' % fn in body('single_pick'), fn
    core = open(os.path.join(CSRC, 'acq_core.h')).read()
    dev = open(os.path.join(CSRC, 'acq_core_dev.h')).read()
    cand = re.search(r'CandMoments batch_cand\(int j, int64_t M, int64_t n, const double\* __restrict__ cq.*?\n}\n', core, flags=re.S).group(0)
    assert 'batch_q(' in cand and 'moments_of_sums(' in cand
    assert 'batch_fold(' in re.search(r'double batch_q\(.*?\n}\n', core, flags=re.S).group(0)
    assert 'pick_scalars(' in re.search(r'double pick_member\(.*?\n}\n', dev, flags=re.S).group(0)
    assert not re.search(r'\b(batch_fold|s2_floored|block_argmax|better|nan_last)\(', src)
