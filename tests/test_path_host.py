"""The host part of the pathwise Thompson draws, no GPU: the workspace walks path_sweep_ws, path_weights_ws and
path_grad_ws (csrc/ws_layout.h) and the arithmetic of the fragment-order weight panel, through the stand-alone program
tests/c/path_ws_check.cpp, against tests/golden/path_ws_layouts.json and against the panel's size by hand.

The program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import json
import os
import subprocess

from test_ws_layout_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
WS_SRC = os.path.join(ROOT, 'tests', 'c', 'path_ws_check.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'path_ws_layouts.json')
SAN = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
NLAYOUTS = 7 * 6 + 4 * 4 * 2 + 3 * 2


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror'] + list(flags) + [WS_SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and p.stderr == '', p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'ws layout ok' and lines[-2] == 'layouts %d' % NLAYOUTS, lines[-3:]
    got = {}
    for ln in lines[:-2]:
        f = ln.split()
        assert f[0] == 'layout' and len(f) == 6, ln
        got.setdefault(f[1], {}).setdefault(f[2], []).append([f[3], int(f[4]), int(f[5])])
    return got


def test_the_workspaces_lie_where_the_recorded_layouts_put_them(tmp_path):
    got = _run(_build(tmp_path, 'path_ws_check', ['-O2']))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(want) == set(got) == {'path_sweep', 'path_weights', 'path_grad'}
    assert got == want
    # the panel by hand: per group of 64 draws, 16 k-steps per 64-row tile, one 64-lane fragment per block of 16 draws
    for tag, regions in want['path_sweep'].items():
        S, nv = (int(x.lstrip('Snv')) for x in tag.split('_'))
        tiles, full, rest = -(-nv // 64), S // 64, S % 64
        words = tiles * 16 * 64 * (4 * full + -(-rest // 16))
        v, frag, total = regions
        assert v == ['v', 0, 8 * S * nv] and frag == ['frag', -(-8 * S * nv // 512) * 512, 8 * words] and total == ['total', 0, frag[1] + frag[2]], tag
    for tag, regions in want['path_weights'].items():
        S, N, eps = (int(x.lstrip('SNeps')) for x in tag.split('_'))
        Np, Sp = -(-N // 128) * 128, -(-S // 128) * 128
        names = [r[0] for r in regions]
        assert names == ['prior'] + (['eps'] if eps else []) + ['R', 'V', 'W', 'v', 'total'], tag
        by = dict((r[0], r) for r in regions)
        assert by['R'][1] % 512 == 0 and by['R'][2] == by['V'][2] == by['W'][2] == 8 * Np * Sp and by['v'][2] == by['prior'][2] == 8 * S * N, tag


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'path_ws_check_san', SAN))


def test_the_library_carves_with_the_header_the_check_includes():
    assert '#include "../../pybo_amd/csrc/ws_layout.h"' in open(WS_SRC).read()
    api = open(os.path.join(CSRC, 'api.hip')).read()
    for call in ('path_sweep_ws(WsCarver(nullptr), S, nv)', 'path_sweep_ws(WsCarver(h->dpath), S, nv)', 'path_weights_ws(WsCarver(nullptr)',
                 'path_weights_ws(WsCarver(h->dpath)'):
        assert call in api, call
    grad = open(os.path.join(CSRC, 'kernels_grad.hip')).read()
    assert 'path_grad_ws(WsCarver(nullptr)' in grad and 'path_grad_ws(WsCarver(h->dpath)' in grad
    assert 'hipFree(h->dpath)' not in api and 'h->dpath}' in api                                   # one ensure, freed with the rest
    kern = open(os.path.join(CSRC, 'kernels_path.hip')).read()
    for fn in ('path_tiles(', 'path_group_blocks(', 'path_group_offset('):                         # the launcher walks the panel by the header's arithmetic
        assert fn in kern, fn
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'kernels_path' in build and 'xgram_core.h' in build
    # the covariance tile is formed by the cross-Gram's own device functions, defined once
    sweep = open(os.path.join(CSRC, 'kernels_sweep.hip')).read()
    hdr = open(os.path.join(CSRC, 'xgram_core.h')).read()
    assert '#include "xgram_core.h"' in sweep and '#include "xgram_core.h"' in kern
    assert 'void dist_step(' in hdr and 'void dist_step(' not in sweep and 'void dist_step(' not in kern
    assert 'xgram_tile_r2(' in sweep and 'xgram_tile_r2(' in kern and 'kern_eval(KID' in kern
