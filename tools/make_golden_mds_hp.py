#!/usr/bin/env python3
"""tests/golden/mds_hp.json: the measured tolerances of the extended-precision MDS tests.

For every case of tests/mds_hp_cases.py the float64 model (tests/mds_oracle.py: direct_D, step, stress) is compared with the
long-double oracle of tests/mds_oracle_hp.py, as |model - oracle| / unit per entry.  Recorded: the SHA-256 of every input, the
ratio per case, per quantity the worst ratio and the case it occurred in, the allowed ratio = 8 x that worst, the oracle's v_t
of the stop cases with their margins and delta, the ratio each mutant of the model reaches on its named cases, and the oracle's
own distance from 50-digit mpmath on three small cases.  Nothing here comes from the device, and this script does not use the
package under test.

    python tools/make_golden_mds_hp.py
"""
import json
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import mds_hp_cases as K  # noqa: E402


def main():
    doc = K.measure()
    doc["oracle_vs_mpmath"] = K.mp_distances()
    with open(K.JSON, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("worst", doc["worst"])
    print("allowed", doc["allowed"], "delta", doc["delta"])
    print("mutants", {k: [(f["case"], f["quantity"], f["over_allowed"]) for f in v["fails"]] for k, v in doc["mutants"].items()})
    print("oracle_vs_mpmath", doc["oracle_vs_mpmath"])


if __name__ == "__main__":
    main()
