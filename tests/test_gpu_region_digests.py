"""The region scorer's bits, pinned: every output column of score_ranges, score_ranges_panel and explain_ranges on the range set
of tests/ranges_cases.py, as SHA-256 digests against tests/golden/region_digests.json (tools/region_digests.py, which computes
both sides).  The kernel headers promise that each column is a function of the range and the profile alone; the file is
regenerated only by a change that means to alter bits."""
import json
import os
import sys

import pytest

import ranges_cases as R
from golden_util import GOLD

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import region_digests as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kmin,kmax", R.ORDERS)
def test_every_column_has_the_recorded_digest(kmin, kmax):
    with open(os.path.join(GOLD, "region_digests.json")) as f:
        want = json.load(f)[D.key(kmin, kmax)]
    got = D.digests(kmin, kmax)
    assert sorted(got) == sorted(want) and len(want) == 2 * (1 + len(D.PANELS) + len(D.TOPS))
    differ = [(case, c) for case in want for c in want[case] if got[case].get(c) != want[case][c]]
    assert not differ, differ
    assert all(sorted(got[case]) == sorted(want[case]) for case in want)
