"""The fantasised batch proposals' workspace (pybo_amd/csrc/ws_layout.h: fant_ws) on the host, against its recorded layout.

tests/c/fant_ws_check.cpp follows tests/c/con_ws_check.cpp: it runs the walk at (M, nb, S) = (1, 1, 1), (3001, 8, 5), (2^20, 64, 64),
checks what it can check alone (sizing walk = carving walk, regions in bounds, pairwise disjoint, aligned as their readers need, the
kernels' furthest reads inside an allocation of exactly the total) and prints every region; here every printed line is held against
tests/golden/fant_ws_layouts.json -- by hand: max(nb - 1, 1) rows of Sp = 16 ceil(S / 16) innovations at 0, Sp incumbents behind them, 64
forced rows behind those.  Nothing grows with M: the per-candidate state is the believer's batch_ws, which test_ws_layout_host.py records
and which the new walk leaves untouched (that test still passes as it is).

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import json
import os
import subprocess

from test_ws_layout_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'fant_ws_check.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fant_ws_layouts.json')
SHAPES = ((1, 1, 1), (3001, 8, 5), (1 << 20, 64, 64))


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


def test_every_region_lies_where_the_recorded_layout_puts_it(tmp_path):
    got = _run(_build(tmp_path, 'fant_ws_check', ['-O2']))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(got) == set(want) == {'fant'}
    assert set(got['fant']) == set(want['fant']) == {'M%d_nb%d_S%d' % s for s in SHAPES}
    for M, nb, S in SHAPES:
        tag = 'M%d_nb%d_S%d' % (M, nb, S)
        assert got['fant'][tag] == want['fant'][tag], tag
        sp, rows = (S + 15) // 16 * 16, max(nb - 1, 1)
        assert want['fant'][tag] == [['eps', 0, 8 * rows * sp], ['t', 8 * rows * sp, 8 * sp], ['pend_idx', 8 * (rows + 1) * sp, 512],
                                     ['total', 0, 8 * (rows + 1) * sp + 512]]
        assert all(off % 128 == 0 for _, off, _ in want['fant'][tag])      # every region starts on a 128-byte line
    # the largest call's innovations and incumbents are what the scoring kernel copies into LDS: 32 KB
    assert want['fant']['M1048576_nb64_S64'][2][1] == 32768


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'fant_ws_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_library_carves_with_the_header_the_check_includes():
    assert '#include "../../pybo_amd/csrc/ws_layout.h"' in open(SRC).read()
    api = open(os.path.join(CSRC, 'api.hip')).read()
    assert 'fant_ws(WsCarver(nullptr), nb, S)' in api and 'fant_ws(WsCarver(h->dfant), nb, S)' in api
    assert 'hipMalloc((void**)&h->dfant' not in api and 'hipFree(h->dfant)' not in api and 'h->dfant,' in api      # one ensure, freed with the rest
    # its own handle pointer: the believer's buffer is carved by the walk it always had
    assert 'batch_ws(WsCarver(h->dbsel), xpad, ld, M, nb, n_lead, ndesc)' in api
