"""The per-candidate arithmetic gives the bits it gave before it got one definition (pybo_amd/csrc/acq_core.h):
tests/golden/acq_digests.json holds, per case of tests/golden/make_acq_digests.py, the SHA-256 of every output (values, moments
and top-k of the cold pi / ucb / mean / mes / kg sweeps, of re-scored caches seeded by ei, mes and kg, the batch picks, the
ensemble's sweeps and batch picks, predictions with gradients) as the library of the recorded commit produced them.  The same
cases run on the current library and must reproduce every digest; every sweep among them also asserts the order's tie rule."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
import make_acq_digests as digests    # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, 'acq_digests.json')) as _f:
    FIXTURE = json.load(_f)
CASES = digests.cases()


def test_the_fixture_records_every_case():
    assert sorted(FIXTURE['cases']) == sorted(name for name, _ in CASES)
    assert len(FIXTURE['commit']) == 40


@pytest.mark.parametrize('name', [name for name, _ in CASES])
def test_outputs_match_the_recorded_digests(name):
    want = FIXTURE['cases'][name]
    got = dict(CASES)[name]()
    assert sorted(got) == sorted(want)
    diff = {k: (v, got[k]) for k, v in want.items() if got[k] != v}
    assert not diff, 'differs from commit %s: %s' % (FIXTURE['commit'][:7], sorted(diff))
