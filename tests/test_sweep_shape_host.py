"""The shape of a sweep launch -- tile width and LDS images (pybo_amd/csrc/sweep_map.h: sweep_shape_of) -- decided on the host, checked on the host.

tests/c/sweep_shape_check.cpp includes the header the launch includes and walks nP in 1 .. 130, nR in {nP, nP / 4, 1}, valid in
1 .. 20000 around every tile boundary, 256 and 304 compute units and every value of the options sweep_cols and sweep_images:
widths and image counts that exist; two images by size exactly where the map's working blocks (walked through sweep_tile_of)
number at most the compute units; with sweep_images = 1 the width of a full launch as it was before the image count existed;
forced options honoured where instances exist and ignored elsewhere; the row-prefix width the one with the fewest weighted
generations; every implied grid total and exact.  An out-of-range tile would be an out-of-bounds write of a kernel.

tests/golden/sweep_cols_full_launch.txt is that earlier rule's table: sweep_cols_of(sweep_cols, tile_order, nP, nP, valid) of the
commit before sweep_shape_of replaced it, evaluated by a host program around that function's text for nP in 1 .. 130, valid in
1 .. 20000, run-length encoded.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'sweep_shape_check.cpp')
TABLE = os.path.join(ROOT, 'tests', 'golden', 'sweep_cols_full_launch.txt')


def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/sweep_shape_check.cpp with')


def _build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror'] + flags + [SRC, '-o', str(exe)])
    p = subprocess.run([str(exe), TABLE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'sweep shapes ok' and len(lines) == 2
    return lines


def test_every_shape_is_legal_and_the_rule_is_what_it_says(tmp_path):
    lines = _build_and_run(tmp_path, 'sweep_shape_check', ['-O2'])
    shapes, two, narrow, grids = [int(part.split()[0]) for part in lines[0].split(', ')]
    assert shapes > 10 ** 7 and two > 0 and narrow > 0 and grids > 10 ** 4       # the walk reached every part of the rule


def test_the_shape_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'sweep_shape_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


def test_the_launch_decides_with_the_header_the_check_includes():
    """One definition of the rule: kernels_sweep.hip calls sweep_shape_of of sweep_map.h and restates neither it nor the thresholds."""
    ksrc = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'kernels_sweep.hip')).read()
    assert 'sweep_shape_of(' in ksrc and 'SweepShape sweep_shape_of' not in ksrc and 'SWEEP_COLS32_MAX' not in ksrc
    assert '#include "../../pybo_amd/csrc/sweep_map.h"' in open(SRC).read()
    hdr = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'sweep_map.h')).read()
    assert 'SweepShape sweep_shape_of(' in hdr and '#include' not in hdr


def test_the_table_of_the_earlier_rule_is_complete():
    rows = [ln.split() for ln in open(TABLE) if not ln.startswith('#')]
    assert all(len(r) == 7 for r in rows)
    by_key = {}
    for to, sc, lo, hi, vlo, vhi, width in (tuple(int(x) for x in r) for r in rows):
        assert width in (32, 64, 128)
        by_key.setdefault((to, sc), []).append((lo, hi, vlo, vhi))
    assert len(by_key) == 12 * 4
    for key, segs in by_key.items():                       # every (nP, valid) of 1 .. 130 x 1 .. 20000 lies in exactly one segment
        assert sum((hi - lo + 1) * (vhi - vlo + 1) for lo, hi, vlo, vhi in segs) == 130 * 20000, key
