"""The device workspaces' one description (pybo_amd/csrc/ws_layout.h) on the host, against the recorded layouts.

tests/c/ws_layout_check.cpp is a stand-alone program around the header the library's host code includes: it runs every workspace's
walk over a fixed list of shapes (d in {1, 3, 8, 18, 19}, Np in {128, 1024, 1152}, a capacity above the current size, M in {1, 127, 1000,
4096, 32768}, k in {1, 4096}, odd and even batch sizes, 1 and 5 draws / features / members, the second bound's rows and the ensemble
lead's words on and off), checks what it can check alone (sizing walk = carving walk, regions in bounds, pairwise disjoint, aligned to
their element type, the alignments the kernels are tuned for, one front for the announcement and the batch buffer) and prints every
region.  Here every printed line is held against tests/golden/ws_layouts.json, which was recorded from the arithmetic of the hand-written
carvings this header replaced: no region moves, no allocation changes its size.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'ws_layout_check.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ws_layouts.json')
LAYOUTS = {'staged', 'ens', 'bound_ops', 'prune', 'keep', 'pend', 'append', 'grad', 'rff_grad', 'spec', 'batch', 'joint', 'kg', 'kg_point',
           'rff_sweep', 'rff_gram', 'rff_wide', 'loglik_batch', 'hyper'}


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/ws_layout_check.cpp with')


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'ws layout ok', lines[-3:]
    got = {}
    for ln in lines[:-2]:
        f = ln.split()
        assert f[0] == 'layout' and len(f) == 6, ln
        got.setdefault(f[1], {}).setdefault(f[2], []).append([f[3], int(f[4]), int(f[5])])
    assert lines[-2] == 'layouts %d' % sum(len(v) for v in got.values())
    return got


def test_every_region_lies_where_the_recorded_layouts_put_it(tmp_path):
    got = _run(_build(tmp_path, 'ws_layout_check', ['-O2']))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(got) == set(want) == LAYOUTS
    for name in sorted(want):
        assert set(got[name]) == set(want[name]), name
        for tag in want[name]:
            assert got[name][tag] == want[name][tag], (name, tag)       # every field in order: name, offset, bytes; the total last
    # the spot values a reader can check by hand against the carvings this replaced (doubles from the base)
    spec = {f: off // 8 for f, off, _ in want['spec']['d8_ld1024_M1000']}
    assert (spec['pscal'], spec['scal'], spec['v'], want['spec']['d8_ld1024_M1000'][-1][2] // 8) == (5248, 5250, 5312, 6312)
    batch = {f: off // 8 for f, off, _ in want['batch']['d8_ld1152_M1000_nb4_lead0']}
    assert (batch['ks'], batch['g'], batch['pscal'], batch['partv'], batch['taken'], batch['V'], batch['ens_s2']) == (128, 1280, 5888, 6272, 10320, 10445, 14445)


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'ws_layout_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_library_carves_with_the_header_the_check_includes():
    assert '#include "../../pybo_amd/csrc/ws_layout.h"' in open(SRC).read()
    hdr = open(os.path.join(CSRC, 'ws_layout.h')).read()
    assert 'hip_runtime' not in hdr and 'gpx_handle' not in hdr and 'hipStream' not in hdr       # plain C++: no HIP type, no handle
    assert '#include "ws_layout.h"' in open(os.path.join(CSRC, 'gpx_internal.h')).read()
    assert 'ws_layout.h' in open(os.path.join(CSRC, 'build.sh')).read()                           # a dependency of the incremental build
    walks = {'api.hip': ('staged_ws(', 'prune_ws_layout(', 'keep_ws(', 'pend_ws(', 'spec_ws(', 'batch_ws(', 'joint_ws(', 'kg_ws(', 'kg_point_ws(',
                         'rff_sweep_ws(', 'rff_gram_ws(', 'rff_wide_ws(', 'ens_ws('),
             'kernels_grad.hip': ('grad_ws(', 'append_ws(', 'rff_grad_ws('), 'kernels_fit.hip': ('loglik_batch_ws(',),
             'kernels_hyper.hip': ('hyper_ws(',), 'kernels_sweep.hip': ('bound_ops(',)}
    # the hand-written formulas are gone, and so is every allocation idiom but the one ensure
    gone = ('2 * xpad + 5 * ld', '(words0 + 3) / 4 * 4', '+ (r.M + r.G) * 8', '+ r.M * 8', '(2 * 4096 + 8) / 2', 'bound_mfma_ws_words', 'nx + 3 * M',
            '2 * B * bs + B * Np * d', 'b.scal + 16 + 46', 'PEND_MAX * (h->cap_np + 2)', '4 * GB * Ncap', 'nW + 2 * nV', 'n * d + 6 * n', '5 * M')
    mallocs = 0
    for name, calls in walks.items():
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "gpx_internal.h"' in src
        for c in calls:
            assert c in src, (name, c)
        for g in gone:
            assert g not in src, (name, g)
        for field in ('dgrad', 'dbatch', 'dhyper', 'dspec', 'dpend', 'dprune', 'dkeep', 'dbsel', 'djoint', 'dkg', 'dkgw', 'drff', 'dens', 'dXc', 'dblki'):
            assert 'hipMalloc((void**)&h->%s' % field not in src and 'hipFree(h->%s)' % field not in src, (name, field)
        mallocs += src.count('int gpx::ensure_bytes(')
    assert mallocs == 1
