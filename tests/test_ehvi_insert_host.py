"""The front insertion of the two-objective batch on the host, no GPU: ehvi_insert (pybo_amd/csrc/ehvi_math.h), the
text the pick kernel k_ehvi_batch_pick runs on the device, through the stand-alone program tests/c/ehvi_insert_check.cpp.  The contract:
starting from ehvi_strips(P, ref) and inserting y_0 .. y_{j-1} in order leaves the arrays of ehvi_strips(P + {y_0 .. y_{j-1}}, ref), bit for
bit -- the program checks that after EVERY insertion, and this file checks the end against the oracle's strips (tests/ehvi_ref.py), exactly:
every output is a copy of an input double.  Streams: the believed outcomes of every case of tests/ehvi_batch_ref.py on its front, random
points over random fronts (lattices too, where coordinates repeat), and the designed ones inside the program (a point equal to a front point,
equal in one coordinate only, on the reference point's edges, below it, dominating the whole front, dominated, into an empty front, growth
to exactly 1024).  Also the workspace walk ehvi_batch_ws (csrc/ws_layout.h) through tests/c/ehvi_batch_ws_check.cpp against
tests/golden/ehvi_batch_ws_layouts.json and by hand.

Both programs are built a second time with -fsanitize=address,undefined and run as plain executables; the first one's arrays hold exactly
the n + 3 and n + 2 doubles the contract asks for."""
import json
import os

import numpy as np
import pytest

import ehvi_batch_ref
import ehvi_ref
from test_ehvi_host import SAN, _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'ehvi_insert_check.cpp')
WS_SRC = os.path.join(ROOT, 'tests', 'c', 'ehvi_batch_ws_check.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ehvi_batch_ws_layouts.json')
OK = 'ehvi insert ok'


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('ehvi_insert'), SRC, 'ehvi_insert_check', ['-O2'])


@pytest.fixture(scope='module')
def san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('ehvi_insert_san'), SRC, 'ehvi_insert_check_san', SAN)


def _stream(exe, tmp_path, P, ref, S):
    """(n after every step, the start included; a; b) of the stream S (ns, 2) inserted into the strips of P over ref."""
    P, S = np.asarray(P, dtype=np.float64).reshape(-1, 2), np.asarray(S, dtype=np.float64).reshape(-1, 2)
    src = str(tmp_path / 'stream.bin')
    np.concatenate([np.asarray(ref, dtype=np.float64).ravel(), [float(len(P))], P.ravel(), S.ravel()]).tofile(src)
    out = _run(exe, OK, 'stream', src)
    ns = [int(f[1]) for f in out if f[0] == 'n']
    a = np.array([float.fromhex(f[1]) for f in out if f[0] == 'a'])
    b = np.array([float.fromhex(f[1]) for f in out if f[0] == 'b'])
    assert len(ns) == len(S) + 1 and len(a) == ns[-1] + 2 and len(b) == ns[-1] + 1
    return ns, a, b


def _equals_the_oracle(P, ref, S, ns, a, b, strips=ehvi_ref.strips):
    wa, wb = strips(np.vstack([np.asarray(P, dtype=float).reshape(-1, 2), np.asarray(S, dtype=float).reshape(-1, 2)]), ref)
    assert ns[-1] == len(wb) - 1
    assert np.array_equal(a.view(np.int64), wa.view(np.int64)) and np.array_equal(b.view(np.int64), wb.view(np.int64))


def test_the_designed_streams(exe):
    assert _run(exe, OK) == []


@pytest.mark.parametrize('tag', sorted(ehvi_batch_ref.CASES))
def test_the_believed_outcomes_of_every_case_inserted_in_order(exe, tmp_path, tag):
    """What the device does between the rounds of this case: n after the first j insertions is the size of the front that scores pick j."""
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case(tag)
    ns, a, b = _stream(exe, tmp_path, P, ref, r['y'][:nb - 1])
    print(tag, ns)
    assert ns == r['n'].tolist() == ehvi_batch_ref.N_PER_ROUND[tag]
    assert np.array_equal(a.view(np.int64), r['strips'][-1][0].view(np.int64)) and np.array_equal(b.view(np.int64), r['strips'][-1][1].view(np.int64))


@pytest.mark.parametrize('seed', range(6))
def test_random_streams_over_random_fronts(exe, tmp_path, seed):
    rng = np.random.RandomState(seed)
    lattice = seed % 2 == 1                     # a coarse lattice: equal points and points equal in one coordinate all the time
    draw = (lambda k: rng.randint(-2, 12, size=(k, 2)) / 4.0) if lattice else (lambda k: rng.rand(k, 2) * 2.0 - 0.3)
    ref = np.array([0.0, 0.25]) if lattice else rng.rand(2) * 0.2
    for np0, ns_ in ((0, 40), (1, 40), (30, 200), (300, 300)):
        P, S = draw(np0), draw(ns_)
        if not lattice and np0 >= 30:          # some of the stream far up and to the right: runs of the front removed at once
            S[::17] = S[::17] * 0.2 + np.array([1.5, 1.5])
        ns, a, b = _stream(exe, tmp_path, P, ref, S)
        _equals_the_oracle(P, ref, S, ns, a, b)
        assert all(n1 <= n0 + 1 for n0, n1 in zip(ns, ns[1:])) and a[0] == ref[0] and a[-1] == np.inf and b[-1] == ref[1]
        assert np.all(np.diff(a) > 0) and np.all(np.diff(b) < 0)
        seen = {(int(n1 - n0) > 0, int(n1 - n0) < -1, n1 == n0) for n0, n1 in zip(ns, ns[1:])}
        if np0 >= 30 and not lattice:          # growth, no change, and a run of at least three points removed
            assert {(True, False, False), (False, False, True), (False, True, False)} <= seen


def test_a_large_front_loses_long_runs(exe, tmp_path):
    """A staircase of 1021 with the stream of the case that removes 900 of its points at once, then a stream that regrows it."""
    p, P, ref, nb, n_obs, r = ehvi_batch_ref.case('se_d8_stair1021')
    assert r['n'][0] - r['n'][1] >= 900
    rng = np.random.RandomState(9)
    S = np.vstack([r['y'], ref + (P.max(0) - ref) * rng.rand(200, 2), np.vstack([P, r['y']]).max(0) + 1.0])
    ns, a, b = _stream(exe, tmp_path, P, ref, S)
    _equals_the_oracle(P, ref, S, ns, a, b, strips=ehvi_batch_ref.strips_vec)
    assert ns[:4] == r['n'].tolist() and ns[-1] == 1 and max(ns) == 1021


def test_the_insertion_is_clean_under_the_address_and_undefined_behaviour_sanitizers(san, tmp_path):
    assert _run(san, OK) == []
    rng = np.random.RandomState(3)
    P, S = rng.rand(50, 2), np.vstack([rng.rand(120, 2), rng.randint(0, 5, size=(60, 2)) / 4.0])
    ns, a, b = _stream(san, tmp_path, P, [0.1, 0.1], S)
    _equals_the_oracle(P, [0.1, 0.1], S, ns, a, b)
    ns, a, b = _stream(san, tmp_path, np.empty((0, 2)), [0.0, 0.0], np.arange(1, 41, dtype=float)[:, None] * [1.0, -1.0] + [0.0, 41.0])
    assert ns == list(range(41))                                                        # growth by one every time: the arrays' last words


def test_the_workspace_lies_where_the_recorded_layout_puts_it(tmp_path):
    out = _run(_build(tmp_path, WS_SRC, 'ehvi_batch_ws_check', ['-O2']), 'ws layout ok')
    assert out[-1] == ['layouts', '4']
    got = {}
    for f in out[:-1]:
        assert f[0] == 'layout' and f[1] == 'ehvi_batch' and len(f) == 6, f
        got.setdefault(f[2], []).append([f[3], int(f[4]), int(f[5])])
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(want) == {'ehvi_batch'} and set(got) == set(want['ehvi_batch']) == {'ld%d' % ld for ld in (2, 3, 66, 1026)}
    for tag, regions in want['ehvi_batch'].items():
        assert got[tag] == regions, tag
        ld = int(tag[2:])
        by_hand = [['a', 0, 8 * ld], ['b', 8 * ld, 8 * ld], ['sel_y', 16 * ld, 1024], ['sel_nfront', 16 * ld + 1024, 512],
                   ['n', 16 * ld + 1536, 4], ['total', 0, 16 * ld + 1544]]
        assert regions == by_hand, tag
    assert _run(_build(tmp_path, WS_SRC, 'ehvi_batch_ws_check_san', SAN), 'ws layout ok')[-1] == ['layouts', '4']


def test_the_kernels_and_the_library_use_the_headers_the_checks_include():
    import re
    assert '#include "../../pybo_amd/csrc/ehvi_math.h"' in open(SRC).read() and '#include "../../pybo_amd/csrc/ws_layout.h"' in open(WS_SRC).read()
    hdr = open(os.path.join(CSRC, 'ehvi_math.h')).read()
    body = hdr[hdr.index('GPX_ACQ_FN int ehvi_insert('):hdr.index('#if defined(GPX_EHVI_DEVICE)')]
    assert 'std::' not in body and 'new ' not in body and 'malloc' not in body                  # the device runs the same text
    bat = open(os.path.join(CSRC, 'kernels_batch.hip')).read()
    assert '#define GPX_EHVI_DEVICE\n#include "ehvi_math.h"' in bat and bat.index('#include "gpx_math.h"') < bat.index('#define GPX_EHVI_DEVICE')
    score = re.search(r'void k_ehvi_batch_score\(.*?\n}\n', bat, flags=re.S).group(0)
    assert 'batch_score_frame(' in score and score.count('ehvi_value(') == 1 and score.count('moments_of_sums(batch_q(') == 2
    assert 'acq_value(' not in score and 'erfc' not in score and 'fp contract' not in bat           # every EI is ehvi_value's: no second one
    pick = re.search(r'void k_ehvi_batch_pick\(.*?\n}\n', bat, flags=re.S).group(0)
    assert 'merge_pick(' in pick and 'pick_member(' in pick and 'pick_gather(' in pick and pick.count('ehvi_insert(') == 1
    everything = '\n'.join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h')))
    assert len(re.findall(r'^GPX_ACQ_FN[^\n(]*\behvi_insert\(', everything, flags=re.M)) == 1      # defined once
    api = open(os.path.join(CSRC, 'api.hip')).read()
    assert 'ehvi_batch_ws(WsCarver(nullptr), EHVI_STRIP_LD)' in api and 'ehvi_batch_ws(WsCarver(L->dehvib), EHVI_STRIP_LD)' in api
    assert 'hipFree(h->dehvib)' not in api and 'h->dehvib,' in api                               # one ensure, freed with the rest
