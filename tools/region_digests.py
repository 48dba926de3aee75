#!/usr/bin/env python3
"""SHA-256 of every output column of the region scorer on the tests' own tiny inputs: the pin of tests/golden/region_digests.json
(tests/test_gpu_region_digests.py recomputes and compares).  Every column is a function of the range and the profile alone
(csrc/range_kernels.h), so the digests move only with a change that means to alter bits - and only such a change regenerates
the file.

Per (kmin, kmax) of ranges_cases.ORDERS and per form (auto / big), on ranges_cases.range_set(kmax) followed by the five rows of
the orphan hand-over test:
  score      Engine.score_ranges under ranges_cases.profile (rip where 2 is within kmin..kmax)
  panel      Engine.score_ranges_panel with panel_cases.profiles at P = 3 (one tile) and P = 9 (two tiles)
  explain    Engine.explain_ranges at top_n = 1, 5 and 64, all thirteen columns

    python tools/region_digests.py > tests/golden/region_digests.json
"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import panel_cases as PC  # noqa: E402
import ranges_cases as R  # noqa: E402

NOTE = ("SHA-256 per output column of the region scorer (tools/region_digests.py).  Regenerated only by a change that means to "
        "alter bits.")
HANDOVER_ROWS = [(2, 0, 640), (2, 0, 650), (2, 0, 65535), (2, 10, 650), (0, 100, 700)]
PANELS = (3, 9)
TOPS = (1, 5, 64)
SCORE = ["status", "nn", "kld", "gc"]
RIP = ["pi", "si", "cri"]
TOP = ["n_present", "code", "count", "pw", "pg", "term"]


def _sha(res, cols):
    return {c: hashlib.sha256(np.ascontiguousarray(getattr(res, c)).tobytes()).hexdigest() for c in cols}


def digests(kmin, kmax):
    """{case: {column: hex digest}} of one (kmin, kmax)."""
    from frisk_amd.engine import Engine
    rip = kmin <= 2 <= kmax
    s, a, b = R.arrays(R.range_set(kmax) + HANDOVER_ROWS)
    score_cols = SCORE + (RIP if rip else [])
    out = {}
    with Engine(kmin, kmax) as e:
        e.load(R.scaffolds())
        PC.install(e, R.profile(kmin, kmax))
        for big in (False, True):
            form = "big" if big else "auto"
            out["score/%s" % form] = _sha(e.score_ranges(s, a, b, rip=rip, big=big), score_cols)
            for top_n in TOPS:
                out["explain/top%d/%s" % (top_n, form)] = _sha(e.explain_ranges(s, a, b, top_n, rip=rip, big=big), score_cols + TOP)
        for P in PANELS:
            e.panel_reset()
            for prof in PC.profiles(P, kmin, kmax):
                PC.install(e, prof)
                e.panel_push()
            for big in (False, True):
                out["panel/P%d/%s" % (P, "big" if big else "auto")] = _sha(e.score_ranges_panel(s, a, b, rip=rip, big=big), score_cols)
    return out


def key(kmin, kmax):
    return "k%d-%d" % (kmin, kmax)


def main():
    doc = {"_note": NOTE}
    for kmin, kmax in R.ORDERS:
        doc[key(kmin, kmax)] = digests(kmin, kmax)
    json.dump(doc, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
