"""The carried gate decision of selection-only sweeps (pybo_amd/csrc/prune_hint.h) on the host.

tests/c/prune_hint_check.cpp includes the header api.hip includes and checks: an unarmed hint matches nothing; an armed one matches
its own key and no key that differs in any one field (kernel, member count, d, block rows, padded rows, M, k); the rule arms at
nsurv = cap / 2 and not at cap / 2 + 1; paths 0, 1 and 3 never arm.

The same program is built a second time with -fsanitize=address,undefined and run as a plain executable."""
import os
import subprocess

from test_bound_exp_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'prune_hint_check.cpp')
CASES = 5


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'prune hint ok %d cases' % CASES and len(lines) == CASES + 1, lines
    return lines[:-1]


def test_matching_and_the_arming_rule(tmp_path):
    lines = _run(_build(tmp_path, 'prune_hint_check', ['-O2']))
    for want in ('unarmed matches nothing', 'armed matches its own key', 'each of 7 key fields decides',
                 'rule at cap / 2 and cap / 2 + 1', 'paths other than 2 never arm'):
        assert want in lines, (want, lines)


def test_the_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path, 'prune_hint_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


def test_the_library_includes_the_header_the_check_includes():
    """One definition of the key, the match and the rule: the handle, both sweep paths and the host program use prune_hint.h.  The
    library consults them in ONE place, the selection driver, and both sweep paths go through that driver."""
    csrc = os.path.join(ROOT, 'pybo_amd', 'csrc')
    hdr = open(os.path.join(csrc, 'prune_hint.h')).read()
    assert 'threadIdx' not in hdr and 'hip_runtime' not in hdr and 'gpx_internal' not in hdr      # plain C++
    assert '#include "prune_hint.h"' in open(os.path.join(csrc, 'gpx_internal.h')).read()
    api = open(os.path.join(csrc, 'api.hip')).read()
    driver = api[api.index('static int select_topk_pruned('):api.index('static int plain_rest(')]
    for call in ('prune_hint_matches(', 'prune_hint_after('):
        assert api.count(call) == 1 and driver.count(call) == 1, call
    assert api.count('select_topk_pruned(') == 4                                      # its definition and the three calls below
    for body, hint in ((api[api.index('static int sweep_core('):api.index('extern "C" int gpx_sweep_dev(')], 'h->prune_hint'),
                       (api[api.index('static int ensemble_core('):api.index('static int ensemble_check(')], 'L->ens_hint')):
        assert body.count('select_topk_pruned(') == 1 and body.count(hint) == 1        # each hands its own hint object to the driver
    # the constrained sweep hands it a local one: it neither reads nor arms the decisions the lead carries for its own sweeps
    body = api[api.index('static int constrained_core('):api.index('extern "C" int gpx_constrained_sweep_dev(')]
    assert body.count('select_topk_pruned(') == 1 and 'PruneHint hint;' in body and 'h->prune_hint' not in body and 'L->ens_hint' not in body
    assert '#include "../../pybo_amd/csrc/prune_hint.h"' in open(SRC).read()
    assert 'prune_hint.h' in open(os.path.join(csrc, 'build.sh')).read()              # a dependency of the incremental build
