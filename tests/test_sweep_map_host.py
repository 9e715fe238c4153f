"""The block -> tile maps of the sweep kernels (pybo_amd/csrc/sweep_map.h) proved on the host, before any launch relies on them.

tests/c/sweep_map_check.cpp includes the header the kernels include and walks, for every order (0 .. 3 and the two short forms of
order 3), RES in {64, 96}, super_m in {1, 2, 4, 8, 16}, NT in 1 .. 70 and 512 and nR in 1 .. 70, the whole grid of sweep_grid
through sweep_tile_of: every tile (mt < nR, nt < NT) exactly once (as a first tile or as an mt2), no tile out of range, no
working block behind the grid, the pairs (nR-1-i, i) with only the odd middle tile alone, and -- for a short form where the
launch chooses it by size -- at most as many idle blocks as working ones.  An out-of-range tile would be an out-of-bounds write
of a kernel, a tile produced twice a race, a missing one a wrong sum: this is the guard against all three.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'sweep_map_check.cpp')


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/sweep_map_check.cpp with')


def _build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-pthread'] + flags + [SRC, '-o', str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'sweep maps ok' and len(lines) == 7
    for order, ln in enumerate(lines[:6]):
        assert ln.startswith('order %d: 49700 launches' % order), ln       # 5 super_m x 71 NT x 70 nR x 2 RES
    return lines


def test_every_map_is_total_and_exact(tmp_path):
    lines = _build_and_run(tmp_path, 'sweep_map_check', ['-O2'])
    # the maps agree on what there is to do: the unpaired ones one block per tile, the paired ones one per pair or lone tile
    working = [int(ln.split(' blocks, ')[1].split(' working')[0]) for ln in lines[:6]]
    assert working[0] == working[1] == working[2] and working[3] == working[4] == working[5] < working[0]


def test_the_map_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'sweep_map_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


def test_the_kernels_include_the_header_the_check_includes():
    """One definition of the maps: kernels_sweep.hip and the host program include sweep_map.h; neither restates it."""
    ksrc = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'kernels_sweep.hip')).read()
    assert '#include "sweep_map.h"' in ksrc and 'bool sweep_tile_of(' not in ksrc and 'sweep_grid(int' not in ksrc
    assert '#include "../../pybo_amd/csrc/sweep_map.h"' in open(SRC).read()
    hdr = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'sweep_map.h')).read()
    assert '#include' not in hdr and 'dim3' not in hdr and 'blockIdx.' not in hdr     # plain C++: no header, no HIP type
