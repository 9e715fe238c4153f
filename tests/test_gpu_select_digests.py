"""Selection-only sweeps decide what they decided before their steps moved into one driver: tests/golden/select_digests.json holds,
per case of tests/golden/make_select_digests.py, every scalar of the device's report, the SHA-256 of the bound vector, the survivor
list, the top-k pairs and (under prune_keep) the kept vectors, and the members' launch and flop counters, as the library of the
recorded commit produced them -- single model and ensemble, forced and automatic (gated, hinted, fell back, declined), and the calls
that must leave an armed hint alone.  The same cases run on the current library and must reproduce every entry."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
import make_select_digests as digests    # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, 'select_digests.json')) as _f:
    FIXTURE = json.load(_f)
CASES = digests.cases()


def test_the_fixture_records_every_case():
    assert sorted(FIXTURE['cases']) == sorted(name for name, _ in CASES)
    assert len(FIXTURE['commit']) == 40


@pytest.mark.parametrize('name', [name for name, _ in CASES])
def test_selection_state_matches_the_recorded_digests(name):
    want = FIXTURE['cases'][name]
    got = dict(CASES)[name]()
    assert sorted(got) == sorted(want)
    diff = {'%s / %s' % (step, k): (v, got[step].get(k)) for step in want for k, v in want[step].items() if got[step].get(k) != v}
    assert not diff, 'differs from commit %s: %s' % (FIXTURE['commit'][:7], sorted(diff.items()))
