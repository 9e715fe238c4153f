"""The shared per-candidate arithmetic (pybo_amd/csrc/acq_core.h) on the host, bit for bit against numpy.

tests/c/acq_core_check.cpp is a stand-alone program around the header the acquisition kernels include.  It prints, in hexadecimal,
inputs and results of: the candidate sums and moments for nrb = 0, 1, 3 over values whose order of addition matters; the ensemble's
fold and finish for n = 1, 2, 3, 10 in both modes; better() over every pair of a set with +-inf, +-0, duplicates and NaN; a pick's
four scalars; the batch fold.  Here every line is recomputed FROM THE DOUBLES PRINTED by the expression the library promises and
compared bit for bit.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ens_batch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'acq_core_check.cpp')
FLOOR = 1e-100


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/acq_core_check.cpp with')


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'acq core ok', lines[-3:]
    return [ln.split() for ln in lines[:-1]]


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp('acq_core'), 'acq_core_check', ['-O2']))


def _f(words):
    return np.array([float.fromhex(w) for w in words], dtype=np.float64)


def _bits(x):
    return struct.pack('<d', float(x))


def _same(got, want):
    """bit for bit; any NaN equals any NaN"""
    return (math.isnan(got) and math.isnan(want)) or _bits(got) == _bits(want)


def _sum_in_order(terms):
    acc = np.float64(0.0)
    for t in terms:
        acc = acc + np.float64(t)
    return acc


def _sum_from_first(terms):
    acc = np.float64(terms[0])
    for t in terms[1:]:
        acc = acc + np.float64(t)
    return acc


def test_sums_and_moments(lines):
    assert _f(next(f for f in lines if f[0] == 'floor')[1:])[0] == FLOOR
    seen, floored = set(), 0
    for f in (f for f in lines if f[0] == 'moments'):
        nrb, ldp, n = int(f[1]), int(f[2]), int(f[3])
        rows = max(nrb, 1)
        v = _f(f[4:])
        rho, bias = v[0], v[1]
        Q, P = v[2:2 + rows * ldp].reshape(rows, ldp), v[2 + rows * ldp:2 + 2 * rows * ldp].reshape(rows, ldp)
        q, p, mu, s2, qR = v[2 + 2 * rows * ldp:]
        want_q = Q[0, n] if nrb == 0 else _sum_in_order(Q[:, n])           # ((0.0 + a) + b) + c
        want_p = P[0, n] if nrb == 0 else _sum_in_order(P[:, n])
        assert _same(q, want_q) and _same(p, want_p), f
        assert _same(qR, _sum_in_order(Q[:nrb, n])), f
        assert _same(mu, np.float64(bias) + want_p), f
        with np.errstate(invalid='ignore'):
            want_s2 = np.fmax(np.float64(rho) - want_q, FLOOR)                 # fmax: a NaN q gives the floor
        assert _same(s2, want_s2) and s2 >= FLOOR, f
        seen.add(nrb)
        floored += int(s2 == FLOOR)
        if nrb == 3 and list(Q[:, n]) == [1e16, 1.0, -1e16]:
            assert q == 0.0                                                # the order matters: 1e16 + 1 rounds the 1 away
        if nrb == 3 and list(Q[:, n]) == [1e16, -1e16, 1.0]:
            assert q == 1.0
    assert seen == {0, 1, 3}
    assert floored >= 6                                                    # q > rho, q = NaN, rho - q = 0 and rho at the floor all occur
    assert any(f[0] == 'moments' and math.isnan(_f(f[-5:])[0]) and _f(f[-5:])[3] == FLOOR for f in lines)


def test_ensemble_fold_and_finish(lines):
    sizes, single = set(), 0
    for f in (f for f in lines if f[0] == 'ens'):
        n, mode = int(f[1]), int(f[2])
        v = _f(f[3:])
        beta, t0, t1 = v[0], v[1:1 + n], v[1 + n:1 + 2 * n]
        value, mu, s2 = v[1 + 2 * n:]
        want_mu = _sum_from_first(t0) / np.float64(n)                      # sum in member order, one division
        assert _same(mu, want_mu), f
        if mode == 0:
            assert _same(value, want_mu) and s2 == 0.0, f
            by_numpy = np.mean(np.stack([t0, t0], axis=1), axis=0)[0]
            assert _same(value, by_numpy), f
        else:
            acc1 = _sum_from_first([b + a * a for a, b in zip(t0, t1)])
            want_s2 = np.maximum(acc1 / np.float64(n) - want_mu * want_mu, 0.0)
            assert _same(s2, want_s2), f
            assert _same(value, want_mu + np.sqrt(np.float64(beta) * want_s2)), f
            # the expression of tests/ens_batch_ref.py, on (n, 2) arrays
            ref, ref_mu, ref_s2 = ens_batch_ref.ensemble_value('ucb', beta, np.stack([t0, t0], axis=1), np.stack([t1, t1], axis=1))
            assert _same(value, ref[0]) and _same(mu, ref_mu[0]) and _same(s2, ref_s2[0]), f
            if n == 1:
                # ONE member in mode 1 is fl(fl(s2 + mu^2) - mu^2), not s2: the single-model batch must never be routed through here
                assert _same(s2, max((t1[0] + t0[0] * t0[0]) - t0[0] * t0[0], 0.0))
                single += int(s2 != t1[0])
        sizes.add(n)
    assert sizes == {1, 2, 3, 10} and single >= 1


def test_the_order_is_a_strict_total_order_with_nan_last(lines):
    f = next(f for f in lines if f[0] == 'orderset')
    n = int(f[1])
    vals, idx = _f(f[2::2]), [int(w) for w in f[3::2]]
    assert len(vals) == len(idx) == n and len(set(idx)) == n
    mat = np.array([[int(c) for c in r[1]] for r in lines if r[0] == 'orderrow'])
    assert mat.shape == (n, n)
    v = np.where(np.isnan(vals), -np.inf, vals)                            # NaN mapped last
    assert np.isnan(vals).sum() == 2 and {0.0, 1.0, np.inf, -np.inf} <= set(v)
    assert any(math.copysign(1.0, x) < 0 and x == 0.0 for x in vals) and any(math.copysign(1.0, x) > 0 and x == 0.0 for x in vals)
    for a in range(n):
        assert mat[a, a] == 0                                              # irreflexive
        for b in range(n):
            want = (v[a] > v[b]) or (v[a] == v[b] and idx[a] < idx[b])     # value descending, index ascending; -0.0 == +0.0
            assert mat[a, b] == int(want), (a, b)
            if a != b:
                assert mat[a, b] + mat[b, a] == 1                          # antisymmetric and total
            for c in range(n):
                if mat[a, b] and mat[b, c]:
                    assert mat[a, c]                                       # transitive
    zeros = [a for a in range(n) if v[a] == 0.0]
    assert len(zeros) == 4 and all(mat[a, b] == int(idx[a] < idx[b]) for a in zeros for b in zeros)     # +-0 tie: the index decides
    assert mat[:, n - 1].sum() == n - 1 and mat[n - 1].sum() == 0          # the "no candidate" pair ranks after everything, NaN included


def test_pick_scalars_and_batch_fold(lines):
    picks = [_f(f[1:]) for f in lines if f[0] == 'pick']
    assert len(picks) == 3
    for s2, sn2, d, invd, zero, d2 in picks:
        assert _same(d2, s2 + sn2) and _same(d, np.sqrt(s2 + sn2)) and _same(invd, 1.0 / np.sqrt(s2 + sn2)) and _bits(zero) == _bits(0.0)
    s2, sn2, d, invd = picks[0][:4]
    assert s2 == FLOOR and sn2 == 0.0 and abs(d - 1e-50) <= 1e-65 and math.isfinite(invd) and abs(invd - 1e50) <= 1e35
    folds = [(int(f[1]), _f(f[2:])) for f in lines if f[0] == 'fold']
    assert [j for j, _ in folds] == [0, 3]
    for j, w in folds:
        invd, vraw, qprev, cross, V, v, q = w[0], w[1], w[2], w[3:6], w[6:9], w[9], w[10]
        t = np.float64(0.0)
        for l in range(j):
            t = t + cross[l] * V[l]                                        # each product rounded before it is added
        want_v = vraw - t * invd
        assert _same(v, want_v) and _same(q, qprev + want_v * want_v), (j, w)


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'acq_core_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_kernels_use_the_header_the_check_includes():
    assert '#include "../../pybo_amd/csrc/acq_core.h"' in open(SRC).read()
    hdr = open(os.path.join(CSRC, 'acq_core.h')).read()
    assert 'threadIdx' not in hdr and 'hip_runtime' not in hdr and '__shfl' not in hdr          # plain C++: no HIP type
    dev = open(os.path.join(CSRC, 'acq_core_dev.h')).read()
    assert '#include "acq_core.h"' in dev
    for name in ('kernels_sweep', 'kernels_mes', 'kernels_kg', 'kernels_batch', 'kernels_ens', 'kernels_grad', 'api'):
        src = open(os.path.join(CSRC, name + '.hip')).read()
        assert '#include "acq_core.h"' in src or '#include "acq_core_dev.h"' in src, name
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'acq_core.h' in build and 'acq_core_dev.h' in build              # dependencies of the incremental build
    # one definition each: the floor's literal only where the constant is defined, the two macros nowhere, one copy of each function
    everything = {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h', '.cpp', '.sh'))}
    floor_lines = [(n, ln) for n, text in everything.items() for ln in text.splitlines() if '1e-100' in ln]
    assert floor_lines == [('acq_core.h', 'constexpr double S2_FLOOR = 1e-100;')]
    for n, text in everything.items():
        assert 'GPX_NEG_INF' not in text and 'GPX_IDX_NONE' not in text, n
    whole = '\n'.join(everything.values())
    for fn in ('better', 'block_argmax', 'batch_fold', 'ens_fold', 'ens_mean', 'ens_value', 'cand_moments', 'merge_pick', 'pick_scalars',
               'ei_mean_bound', 'acq_frame', 's2_floored'):
        assert len(re.findall(r'^(?:GPX_ACQ_FN|__device__ __forceinline__)[^\n(]*\b%s\(' % fn, whole, flags=re.M)) == 1, fn
