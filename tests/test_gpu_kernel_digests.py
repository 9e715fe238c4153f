"""The kernels give the bits they gave before they were folded together: tests/golden/kernel_digests.json holds, per case of
tests/golden/make_kernel_digests.py, the SHA-256 of every output (the factor, its inverse and the solve vectors for five sizes
under both association orders of the inverse, with and without its leading part riding behind the factorisation, once
refined, and at N = 1000 with the factorisation's workers forced onto their one-image and their two-image k-loop (chol_tg_db
0 / 1: the default takes the two-image one at every size here); the sweep's values, moments and top-k under every k-loop schedule; one RFF sweep) as the library of the recorded
commit produced them.  The same cases run on the current library and must reproduce every digest."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
import make_kernel_digests as digests    # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, 'kernel_digests.json')) as _f:
    FIXTURE = json.load(_f)
CASES = digests.cases()


def test_the_fixture_records_every_case():
    assert sorted(FIXTURE['cases']) == sorted(name for name, _ in CASES)
    assert len(FIXTURE['commit']) == 40


@pytest.mark.parametrize('name', [name for name, _ in CASES])
def test_kernel_outputs_match_the_recorded_digests(name):
    want = FIXTURE['cases'][name]
    got = dict(CASES)[name]()
    if name.startswith('sweep'):            # {schedule: {output: digest}}: name the schedules and outputs that differ
        diff = {'%s / %s' % (sched, k): (v, got[sched][k]) for sched in want for k, v in want[sched].items() if got[sched][k] != v}
    else:
        diff = {k: (v, got[k]) for k, v in want.items() if got[k] != v}
    assert not diff, 'differs from commit %s: %s' % (FIXTURE['commit'][:7], sorted(diff))
