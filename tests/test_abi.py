"""CPU-side checks of the drop-in boundary: the shared library loads, exports every symbol
include/gpx.h declares, and fails LOUDLY when there is no GPU (no silent fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'gpx.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(gpx_[a-z_0-9]+)\s*\(', src)))


def _declared_diag():
    src = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'gpx_diag.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(gpx_[a-z_0-9]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from pybo_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), 'libgpx.so does not export %s' % n
    # and the binding table covers the header exactly
    assert sorted(_lib.SYMBOLS) == names
    assert sorted(_lib.DIAG_SYMBOLS) == _declared_diag()


def test_shipping_and_diagnostics_builds_export_the_same_abi():
    """build.sh links two libraries from the same objects but diag_flag.cpp (compiled without / with -DGPX_DIAGNOSTICS): both export every
    symbol of include/gpx.h and csrc/gpx_diag.h; gpx_diagnostics() tells them apart; the header stays within its size budget."""
    from pybo_amd import _lib
    libdir = os.path.join(ROOT, 'pybo_amd', 'csrc')
    ship, diag = C.CDLL(os.path.join(libdir, 'libgpx.so')), C.CDLL(os.path.join(libdir, 'libgpx_diag.so'))
    for n in list(_lib.SYMBOLS) + list(_lib.DIAG_SYMBOLS):
        assert hasattr(ship, n) and hasattr(diag, n), n
    assert ship.gpx_diagnostics() == 0 and diag.gpx_diagnostics() == 1
    assert ship.gpx_version() == diag.gpx_version() >= 600
    assert os.path.basename(_lib.LIB_PATH) == 'libgpx_diag.so'          # what this test session drives (conftest.py)
    lines = open(os.path.join(ROOT, 'include', 'gpx.h')).read().splitlines()
    assert len(lines) <= 300 and max(len(ln) for ln in lines) <= 160
    # no diagnostic option is documented as part of the shipping ABI's option list
    public = re.sub(r'Diagnostic knobs.*?GPX_EARG\.', '', open(os.path.join(ROOT, 'include', 'gpx.h')).read(), flags=re.S)
    for name in ('x_skip', 'x_bg', 'chol_tg_chunks', 'chol_tg_nap', 'chol_tg_grid', 'chol_tg_isolate', 'chol_tg_trace', 'grad_rb_cs'):
        assert '"%s"' % name not in public, name


# what test_shipping_library_refuses_the_diagnostic_options offers the shipping library (every one must be refused)
DIAG_PROBES = (('x_skip', 1), ('x_bg', 4), ('x_bg_lds', 8), ('x_bg_iters', 10), ('chol_tg_chunks', 1248), ('chol_tg_nap', 8),
               ('chol_tg_grid', 64), ('chol_tg_isolate', 0), ('chol_tg_trace', 1), ('grad_rb_cs', 128), ('x_rff', 1), ('prune_keep', 1))


def _option_table():
    """{name: diagnostic-only} from the rows of gpx_set_option's table in api.hip."""
    src = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'api.hip')).read()
    rows = re.findall(r'^\s*\{"([a-z0-9_]+)", (SHIP|DIAG),', src, flags=re.M)
    return {name: flag == 'DIAG' for name, flag in rows}


def test_option_table_agrees_with_the_headers():
    """The option table in api.hip is the one list of options: every shipping row is documented in include/gpx.h, the
    diagnostic rows are exactly the options gpx_diag.h documents, the shipping library's refusal test asks for diagnostic
    rows only, and no preprocessor test of GPX_DIAGNOSTICS is left in api.hip (diag_flag.cpp is the only difference)."""
    table = _option_table()
    assert len(table) >= 30
    public = open(os.path.join(ROOT, 'include', 'gpx.h')).read()
    for name, diag in table.items():
        assert diag or '"%s"' % name in public, name
    quoted = set(re.findall(r'"([a-z][a-z0-9_]*)"', open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'gpx_diag.h')).read()))
    assert {name for name, diag in table.items() if diag} == quoted
    assert {name for name, _ in DIAG_PROBES} <= {name for name, diag in table.items() if diag}
    src = open(os.path.join(ROOT, 'pybo_amd', 'csrc', 'api.hip')).read()
    assert not re.search(r'^\s*#\s*if.*GPX_DIAGNOSTICS', src, flags=re.M)


@pytest.mark.gpu
def test_shipping_library_refuses_the_diagnostic_options():
    """A handle of the SHIPPING library answers every diagnostic knob with GPX_EARG (and keeps working); the diagnostics build
    accepts them.  Both libraries live in this process side by side."""
    from pybo_amd import _lib
    ship = C.CDLL(os.path.join(ROOT, 'pybo_amd', 'csrc', 'libgpx.so'))
    ship.gpx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    ship.gpx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    ship.gpx_last_error.restype = C.c_char_p
    ship.gpx_last_error.argtypes = [C.c_void_p]
    ship.gpx_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert ship.gpx_create(0, None, C.byref(h)) == 0
    for name, val in DIAG_PROBES:
        assert ship.gpx_set_option(h, name.encode(), val) == _lib.GPX_EARG, name
        assert b'GPX_DIAGNOSTICS' in ship.gpx_last_error(h)
    for name, val in (('chunk', 256), ('tile_order', 27), ('chol_tg', 0), ('chol_tg_min', 3), ('eager_inverse', 1)):
        assert ship.gpx_set_option(h, name.encode(), val) == 0, name
    assert ship.gpx_destroy(h) == 0
    e = _lib.Engine(0)                                   # the diagnostics build (this session's library)
    for name, val in (('chol_tg_chunks', 1248), ('chol_tg_nap', 8), ('chol_tg_trace', 1), ('x_skip', 0)):
        e.set_option(name, val)
    e.close()


def test_version_and_loud_failure_without_gpu(gpu_available):
    from pybo_amd import _lib
    lib = _lib.load()
    assert lib.gpx_version() >= 100
    if gpu_available:
        pytest.skip('a GPU is present; the no-GPU failure path is checked on CPU-only hosts')
    h = C.c_void_p()
    rc = lib.gpx_create(0, None, C.byref(h))
    assert rc == _lib.GPX_EHIP and not h.value
    assert b'no HIP device' in lib.gpx_last_error(None)
    with pytest.raises(_lib.GpxError):
        _lib.Engine(0)
    # the model object has no CPU path either
    from pybo_amd import models
    gp = models.make_gp(1e-3, 1.0, [0.3, 0.3], 0.0)
    with pytest.raises(_lib.GpxError):
        gp.add_data(np.random.rand(4, 2), np.random.rand(4))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'pybo_amd')
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle', txt, flags=re.M), f


def test_header_is_plain_c_and_links_from_c(tmp_path):
    """The boundary is a C ABI: include/gpx.h compiles as strict C99 and a C program linked against
    libgpx.so can call it (here only gpx_version / gpx_last_error: no device work on a CPU-only host)."""
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no C compiler on this host')
    libdir = os.path.join(ROOT, 'pybo_amd', 'csrc')
    src = tmp_path / 'abi_probe.c'
    src.write_text('#include <stdio.h>\n#include "gpx.h"\n'
                   'int main(void) {\n'
                   '    gpx_handle *h = 0; gpx_grid *g = 0;\n'
                   '    const char *msg = gpx_last_error(0);\n'
                   '    printf("%d %d\\n", gpx_version(), (int)(msg != 0));\n'
                   '    return (h == 0 && g == 0 && GPX_OK == 0 && GPX_GRID_SOBOL == 1) ? 0 : 1;\n'
                   '}\n')
    exe = tmp_path / 'abi_probe'
    subprocess.check_call([gcc, '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic',
                           '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe),
                           '-L', libdir, '-lgpx', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib'])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert int(out[0]) >= 100 and out[1] == '1'

