"""The host parts of the two-objective sweep, no GPU: (a) ehvi_strips (pybo_amd/csrc/ehvi_math.h) through the
stand-alone program tests/c/ehvi_check.cpp against its Python twin pareto.strips -- exactly: every output is a copy of an input double;
(b) ehvi_fold_term against the same statements in numpy, bit for bit; (c) the workspace walk ehvi_ws (csrc/ws_layout.h) through
tests/c/ehvi_ws_check.cpp against tests/golden/ehvi_ws_layouts.json and against the layout by hand: mu1, s2_1, mu2, s2_2, out of 8 M bytes
each, then a and b of 8 (n + 2) bytes each.

Both programs are built a second time with -fsanitize=address,undefined and run as plain executables."""
import json
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from test_ws_layout_host import _compiler
from pybo_amd import pareto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'ehvi_check.cpp')
WS_SRC = os.path.join(ROOT, 'tests', 'c', 'ehvi_ws_check.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ehvi_ws_layouts.json')
SAN = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _build(directory, src, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags) + [src, '-o', exe])
    return exe


def _run(exe, last, *args):
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == last, lines[-3:]
    return [ln.split() for ln in lines[:-1]]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('ehvi'), SRC, 'ehvi_check', ['-O2'])


def _strips(exe, tmp_path, P, ref):
    src = str(tmp_path / 'pts.bin')
    np.concatenate([np.asarray(ref, dtype=np.float64).ravel(), np.asarray(P, dtype=np.float64).ravel()]).tofile(src)
    out = _run(exe, 'ehvi ok', 'strips', src)
    n = int(out[0][1])
    assert out[0][0] == 'n' and len(out) == 1 + (n + 2) + (n + 1)
    a = np.array([float.fromhex(f[1]) for f in out[1:n + 3]])
    b = np.array([float.fromhex(f[1]) for f in out[n + 3:]])
    assert all(f[0] == 'a' for f in out[1:n + 3]) and all(f[0] == 'b' for f in out[n + 3:])
    return n, a, b


def _big(n_front, seed):
    """4096 raw points over ref = (0, 0) of which exactly n_front survive: a staircase, its duplicates, dominated points and points on and
    below the reference point, shuffled."""
    rng = np.random.RandomState(seed)
    i = np.arange(1, n_front + 1, dtype=float)
    front = np.column_stack([i, n_front + 1 - i])
    rest = 4096 - n_front
    pick = rng.randint(0, n_front, size=rest)
    how = rng.randint(0, 4, size=rest)
    extra = front[pick].copy()
    extra[how == 1] -= 0.5                                   # dominated by the point it came from
    extra[how == 2, 0] = 0.0                                 # on the reference point's edge
    extra[how == 3] *= -1.0                                  # below it
    P = np.vstack([front, extra])
    return P[rng.permutation(len(P))]


POINT_SETS = {
    'empty': (np.empty((0, 2)), [0.0, 0.0], 0),
    'one': ([[1.0, 2.0]], [0.0, 0.0], 1),
    'one_below': ([[1.0, 2.0]], [1.5, 0.0], 0),
    'duplicates': ([[1.0, 2.0], [1.0, 2.0], [2.0, 1.0], [1.0, 2.0], [2.0, 1.0]], [0.0, 0.0], 2),
    'equal_f1': ([[1.0, 2.0], [1.0, 3.0], [1.0, 1.0], [2.0, 0.5]], [0.0, 0.0], 2),
    'equal_f2': ([[1.0, 2.0], [3.0, 2.0], [2.0, 2.0], [0.5, 4.0]], [0.0, 0.0], 2),
    'on_and_below_ref': ([[0.0, 5.0], [5.0, 0.0], [-1.0, 9.0], [1.0, 1.0], [0.0, 0.0], [2.0, -3.0]], [0.0, 0.0], 1),
    'negative_ref': ([[-3.0, -1.0], [-2.0, -2.0], [-1.0, -3.0], [-2.5, -2.5], [-5.0, -1.0]], [-4.0, -4.0], 3),
    'raw4096_front1024': (_big(1024, 1), [0.0, 0.0], 1024),
    'raw4096_front1025': (_big(1025, 2), [0.0, 0.0], 1025),
}


@pytest.mark.parametrize('name', sorted(POINT_SETS))
def test_strips_equal_the_python_twin_exactly(exe, tmp_path, name):
    P, ref, want_n = POINT_SETS[name]
    P = np.asarray(P, dtype=float).reshape(-1, 2)
    n, a, b = _strips(exe, tmp_path, P, ref)
    pa, pb = pareto.strips(P, ref)
    assert n == want_n == len(pb) - 1
    assert np.array_equal(a.view(np.int64), pa.view(np.int64)) and np.array_equal(b.view(np.int64), pb.view(np.int64))
    assert a[0] == ref[0] and a[-1] == np.inf and b[-1] == ref[1]
    assert np.all(np.diff(a) > 0) and np.all(np.diff(b) < 0)
    # the survivors are the non-dominated raw points above ref, once each
    above = P[(P[:, 0] > ref[0]) & (P[:, 1] > ref[1])]
    if len(above) <= 64:         # (by the definition, quadratic)
        keep = {tuple(p) for p in above if not any(q[0] >= p[0] and q[1] >= p[1] and tuple(q) != tuple(p) for q in above)}
        assert {(x, y) for x, y in zip(a[1:-1], b[:-1])} == keep
    assert pareto.pareto_mask(above).sum() == n


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def _term(acc, ep, en, e2):
    """ehvi_fold_term's statements in numpy"""
    with np.errstate(invalid='ignore', over='ignore'):
        dif = ep - en
        w = np.where(dif < 0.0, 0.0, dif)
        t = w * e2
        return acc + t


def test_fold_term_on_the_designed_grid(exe):
    lines = [f for f in _run(exe, 'ehvi ok') if f[0] == 'term']
    assert len(lines) == 4 * 11 * 11 * 7
    seen = set()
    for f in lines:
        acc, ep, en, e2, r = (float.fromhex(x) for x in f[1:])
        want = float(_term(np.float64(acc), np.float64(ep), np.float64(en), np.float64(e2)))
        assert (math.isnan(r) and math.isnan(want)) or struct.pack('<d', r) == struct.pack('<d', want), f
        seen.add((ep < en, math.isnan(ep) or math.isnan(en), e2 == np.inf and ep == en))
    assert (True, False, False) in seen and (False, True, False) in seen and (False, False, True) in seen      # negative difference, NaN, 0 * inf


def test_fold_term_on_drawn_inputs_bit_for_bit(exe, tmp_path):
    rng = np.random.RandomState(5)
    m = 200000
    rows = np.exp(rng.uniform(-700.0, 30.0, size=(m, 4)))
    rows[rng.rand(m) < 0.2, 2] *= 4.0                        # e_next above e_prev more often: the clamp
    rows[rng.rand(m) < 0.1, 0] = 0.0
    rows[rng.rand(m) < 0.01, rng.randint(0, 4)] = np.nan
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    rows.tofile(src)
    out = _run(exe, 'ehvi ok', 'fold', src, dst)
    assert out[-1] == ['rows', str(m)]
    got = np.fromfile(dst, dtype=np.float64)
    assert _same_bits(got, _term(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]))
    # a whole chain through the compiled term is pareto.ehvi_from_moments' accumulation
    acc = np.zeros(7)
    e1 = np.sort(rng.rand(6, 7), axis=0)[::-1]
    e2 = rng.rand(6, 7)
    for i in range(6):
        step = np.column_stack([acc, e1[i], e1[i + 1] if i < 5 else np.zeros(7), e2[i]])
        step.tofile(src)
        _run(exe, 'ehvi ok', 'fold', src, dst)
        acc = np.fromfile(dst, dtype=np.float64)
    want = np.zeros(7)
    for i in range(6):
        want = want + np.maximum(e1[i] - (e1[i + 1] if i < 5 else 0.0), 0.0) * e2[i]
    assert _same_bits(acc, want)


def test_the_workspace_lies_where_the_recorded_layout_puts_it(tmp_path):
    p = subprocess.run([_build(tmp_path, WS_SRC, 'ehvi_ws_check', ['-O2'])], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and p.stderr == '', p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'ws layout ok' and lines[-2] == 'layouts 20'
    got = {}
    for ln in lines[:-2]:
        f = ln.split()
        assert f[0] == 'layout' and f[1] == 'ehvi' and len(f) == 6, ln
        got.setdefault(f[2], []).append([f[3], int(f[4]), int(f[5])])
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(want) == {'ehvi'} and set(got) == set(want['ehvi']) == {'M%d_n%d' % (m, n) for m in (1, 257, 4096, 13001, 1048576) for n in (0, 1, 7, 1024)}
    for tag, regions in want['ehvi'].items():
        assert got[tag] == regions, tag
        m, n = (int(x[1:]) for x in tag.split('_'))
        by_hand = [[name, 8 * m * i, 8 * m] for i, name in enumerate(('mu1', 's2_1', 'mu2', 's2_2', 'out'))]
        by_hand += [['a', 40 * m, 8 * (n + 2)], ['b', 40 * m + 8 * (n + 2), 8 * (n + 2)], ['total', 0, 40 * m + 16 * (n + 2)]]
        assert regions == by_hand, tag


def test_the_checks_are_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path, SRC, 'ehvi_check_san', SAN)
    _run(san, 'ehvi ok')
    for name in ('empty', 'duplicates', 'raw4096_front1025'):
        P, ref, want_n = POINT_SETS[name]
        assert _strips(san, tmp_path, P, ref)[0] == want_n
    rows = np.column_stack([np.zeros(8), np.linspace(0.0, 2.0, 8), np.linspace(1.0, 0.0, 8), np.ones(8)])
    rows.tofile(str(tmp_path / 'in.bin'))
    _run(san, 'ehvi ok', 'fold', str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin'))
    ws = _build(tmp_path, WS_SRC, 'ehvi_ws_check_san', SAN)
    assert _run(ws, 'ws layout ok')[-1] == ['layouts', '20']


def test_the_kernel_and_the_library_use_the_headers_the_checks_include():
    import re
    assert '#include "../../pybo_amd/csrc/ehvi_math.h"' in open(SRC).read() and '#include "../../pybo_amd/csrc/ws_layout.h"' in open(WS_SRC).read()
    hdr = open(os.path.join(CSRC, 'ehvi_math.h')).read()
    assert 'hip_runtime' not in hdr and 'threadIdx' not in hdr
    kern = open(os.path.join(CSRC, 'kernels_ehvi.hip')).read()
    assert '#include "ehvi_math.h"' in kern and '#include "gpx_math.h"' in kern and 'ehvi_value(' in kern
    assert 'erfc' not in kern and 'erfc' not in hdr and hdr.count('acq_value(GPX_ACQ_EI') == 3      # every EI is gpx_math.h's: no second implementation
    api = open(os.path.join(CSRC, 'api.hip')).read()
    assert 'ehvi_strips(' in api and 'ehvi_ws(WsCarver(nullptr), M, n)' in api and 'ehvi_ws(WsCarver(L->dehvi), M, n)' in api
    assert 'hipFree(h->dehvi)' not in api and 'h->dehvi,' in api                                  # one ensure, freed with the rest
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'kernels_ehvi' in build and 'ehvi_math.h' in build
    everything = '\n'.join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h')))
    assert len(re.findall(r'^GPX_ACQ_FN[^\n(]*\behvi_fold_term\(', everything, flags=re.M)) == 1
    assert len(re.findall(r'\behvi_fold_term\(', kern)) == 0 and hdr.count('= ehvi_fold_term(') == 1      # the loop's one call
