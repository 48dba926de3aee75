#!/usr/bin/env python3
"""tests/golden/ipca_hp.json: the measured tolerance of the per-entry IncrementalPCA tests.

For every case of tests/ipca_hp_cases.py the float64 restatement of tests/ipca_oracle.py (mean_var_update, stacked, A.T @ A,
transform) is compared with the long-double oracle of tests/ipca_oracle_hp.py, as |restatement - oracle| / unit per entry.
Recorded: the ratios per case, the worst per quantity (G, mean, var, Y), the tolerance = 8 x that worst ratio, the oracle's own
distance from 50-digit mpmath on three small cases in the same units, and for each of the seven planted defects of
ipca_hp_cases.restate its worst ratio / tolerance per quantity and the case that shows it.  Nothing here comes from the device, and
this script does not use the package under test.

    python tools/make_golden_ipca_hp.py
"""
import json
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import ipca_hp_cases as K  # noqa: E402
import ipca_oracle_hp as HP  # noqa: E402


def measure():
    cases = {c.id: K.compare(c.id, K.restate(c.id)) for c in K.CASES}
    worst = {q: max(r[q] for r in cases.values()) for q in K.QUANTITIES}
    return cases, worst


def defect_table(tolerance):
    table = {}
    for defect in K.DEFECTS:
        best = {q: (0.0, None) for q in K.QUANTITIES}
        for c in K.CASES:
            for q, v in K.compare(c.id, K.restate(c.id, defect)).items():
                if v / tolerance[q] > best[q][0]:
                    best[q] = (min(v / tolerance[q], 1e300), c.id)
        table[defect] = {q: {"ratio_over_tolerance": best[q][0], "case": best[q][1]} for q in K.QUANTITIES}
    return table


def mp_distances():
    out = {}
    for cid in K.MP_CASES:
        i = K.inputs(cid)
        st = i.state or {"n": 0, "mean": None, "var": None, "S": None, "Vt": None}
        out[cid] = HP.distance_from_mp(i.Xb, st["n"], st["mean"], st["var"], st["S"], st["Vt"], i.Vt_new)
    return out


def main():
    cases, worst = measure()
    tolerance = {q: K.FACTOR * worst[q] for q in K.QUANTITIES}
    corr, cross = K.assert_shares()
    doc = {"factor": K.FACTOR, "unit_eps": 2.0 ** -52, "quantities": list(K.QUANTITIES), "worst": worst, "tolerance": tolerance,
           "oracle_vs_mpmath": mp_distances(), "defects": defect_table(tolerance),
           "shares": {"correction_row_of_trace_G": {"share": corr[0], "case": corr[1]},
                      "cross_term_of_var": {"share": cross[0], "case": cross[1]}},
           "cases": cases}
    with open(K.JSON, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("worst", worst)
    print("tolerance", tolerance)
    print("oracle_vs_mpmath", doc["oracle_vs_mpmath"])
    for d, t in doc["defects"].items():
        print(d, {q: "%.3g" % v["ratio_over_tolerance"] for q, v in t.items()})
    print("shares", doc["shares"])


if __name__ == "__main__":
    main()
