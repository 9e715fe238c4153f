"""The host-side contract of the C-ABI stays put: tests/golden/api_contract.json holds what gpx_set_option (every option
name, every boundary value), gpx_create under GPX_OPTIONS, and the sweep / ensemble / RFF wrappers (one bad argument at a
time) answered in both libraries before the option table and the shared staging replaced the hand-written checks.  The
same probes (tests/golden/make_api_contract.py) run against the current libgpx.so and libgpx_diag.so, loaded side by side
in this process, and must give identical return codes and messages."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
import make_api_contract as contract    # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('lib', ['ship', 'diag'])
def test_api_contract_matches_the_recorded_one(lib):
    with open(os.path.join(GOLDEN, 'api_contract.json')) as f:
        fixture = json.load(f)
    assert fixture['values'] == contract.VALUES
    want = contract.decode(fixture)[lib]
    path = os.path.join(ROOT, 'pybo_amd', 'csrc', 'libgpx.so' if lib == 'ship' else 'libgpx_diag.so')
    got = contract.probe(path)
    assert sorted(got) == sorted(want)
    diff = {case: (want[case], got[case]) for case in want if got[case] != want[case]}
    assert not diff, diff
