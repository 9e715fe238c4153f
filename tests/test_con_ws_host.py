"""The constrained sweep's workspace (pybo_amd/csrc/ws_layout.h: con_ws) on the host, against its recorded layout.

tests/c/con_ws_check.cpp follows tests/c/ws_layout_check.cpp: it runs the walk over M in {1, 127, 1000, 4096, 13001, 32768}, checks what
it can check alone and prints every region; here every printed line is held against tests/golden/con_ws_layouts.json -- by hand: the
probabilities of one constraint at 0 and the running product at 8 M, 16 M bytes in all.  The layouts test_ws_layout_host.py records
are untouched by the new walk (that test still passes as it is).

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import json
import os
import subprocess

from test_ws_layout_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'con_ws_check.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'con_ws_layouts.json')


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
    got = _run(_build(tmp_path, 'con_ws_check', ['-O2']))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(got) == set(want) == {'con'}
    assert set(got['con']) == set(want['con']) == {'M%d' % m for m in (1, 127, 1000, 4096, 13001, 32768)}
    for tag in want['con']:
        assert got['con'][tag] == want['con'][tag], tag
        m = int(tag[1:])
        assert want['con'][tag] == [['t0', 0, 8 * m], ['out', 8 * m, 8 * m], ['total', 0, 16 * m]]


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'con_ws_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_library_carves_with_the_header_the_check_includes():
    assert '#include "../../pybo_amd/csrc/ws_layout.h"' in open(SRC).read()
    api = open(os.path.join(CSRC, 'api.hip')).read()
    assert 'con_ws(WsCarver(nullptr), M)' in api and 'con_ws(WsCarver(L->dcon), M)' in api
    assert 'hipMalloc((void**)&h->dcon' not in api and 'hipFree(h->dcon)' not in api and 'h->dcon,' in api      # one ensure, freed with the rest
