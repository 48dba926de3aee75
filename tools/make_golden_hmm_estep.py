#!/usr/bin/env python3
"""Golden data of the E-step tests (tests/hmm_estep_cases.py): everything here is measured on the CPU, nothing on a GPU.

1. tests/golden/hmm_estep/large.npz: for every case of 4095 windows and more, the extended-precision oracle's nine statistics and
   its posteriors at the fixed sample of windows (hmm_estep_cases.sample_windows), rounded to float64.
2. tests/golden/hmm_estep.json: the models (data), every input's sha256, the error against the oracle of the float64 piece model
   in the device's layout (tests/hmm_piece_model.py) and of the host-native frisk_hmm_estep on every case, the tolerance
   = FACTOR x the largest of those per quantity, and the oracle's own distance from mpmath (50 digits) on every case of at most
   200 windows, plus the float64 rounding of the recorded / returned reference values.

    python tools/make_golden_hmm_estep.py [--jobs 8]
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import hmm_estep_cases as E  # noqa: E402
import hmm_gpu_cases as H  # noqa: E402
import hmm_oracle_hp as O  # noqa: E402
import hmm_piece_model as PM  # noqa: E402

# rounding of the oracle's long doubles to the float64 the tests compare with: half an ulp - of a value <= 1, absolutely, for a
# posterior; relatively for the others
ROUNDING = {"posterior": 2.0 ** -54, "statistics": 2.0 ** -53, "loglik": 2.0 ** -53}


def one(case):
    model, family, n = case
    x = E.case_input(model, family, n)
    post, stats, ll = O.e_step(x, E.MODELS[model])
    win = E.sample_windows(n) if n in E.LARGE else None
    ref = (win, (post if win is None else post[win]).astype(np.float64), stats.astype(np.float64), float(ll))
    out = {"n": n, "sha256": H.sha(x)}
    out["piece_model"], _ = E.errors(n, PM.e_step(x, E.MODELS[model]), ref)
    out["host"], _ = E.errors(n, E.host_e_step(model, x), ref)
    if n <= 200:
        out["oracle_vs_mpmath"] = dict(zip(E.QUANTITIES, O.distance_from_mp(x, E.MODELS[model])))
        lp, ls, lll = O.e_step_logspace(x, E.MODELS[model])
        out["oracle_vs_logspace"], _ = E.errors(n, (lp.astype(np.float64), ls.astype(np.float64), float(lll)), ref)
    print("%-28s piece model %.2g %.2g %.2g   host %.2g %.2g %.2g" % ((E.case_id(*case),) + tuple(out["piece_model"][q] for q in E.QUANTITIES)
                                                                      + tuple(out["host"][q] for q in E.QUANTITIES)), flush=True)
    large = None if win is None else (ref[1], np.concatenate((ref[2], [ref[3]])))
    return E.case_id(*case), out, large


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    cases = E.all_cases(E.LARGE)[::-1] + E.all_cases(E.SMALL)        # (the slow ones first)
    with multiprocessing.Pool(a.jobs) as pool:
        results = pool.map(one, cases, chunksize=1)
    doc = {"factor": E.FACTOR, "oracle_margin": E.ORACLE_MARGIN, "models": E.MODELS, "small": list(E.SMALL), "large": list(E.LARGE),
           "cases": {}, "error": {}, "oracle_vs_mpmath": {}, "oracle_vs_logspace": {}, "float64_rounding_of_the_reference": ROUNDING}
    arrays = {}
    for cid, out, large in sorted(results, key=lambda r: r[0]):
        doc["cases"][cid] = out
        if large is not None:
            arrays[cid + "/post"], arrays[cid + "/stats"] = large
    for who in ("piece_model", "host"):
        doc["error"][who] = {q: max(c[who][q] for c in doc["cases"].values()) for q in E.QUANTITIES}
    for who in ("oracle_vs_mpmath", "oracle_vs_logspace"):
        doc[who] = {q: max(c[who][q] for c in doc["cases"].values() if who in c) for q in E.QUANTITIES}
    doc["tolerance"] = {q: E.FACTOR * max(doc["error"]["piece_model"][q], doc["error"]["host"][q]) for q in E.QUANTITIES}
    for q in E.QUANTITIES:
        assert E.ORACLE_MARGIN * (doc["oracle_vs_mpmath"][q] + ROUNDING[q]) <= doc["tolerance"][q], (q, doc["oracle_vs_mpmath"], doc["tolerance"])
    os.makedirs(os.path.dirname(E.NPZ), exist_ok=True)
    np.savez_compressed(E.NPZ, **arrays)
    with open(E.JSON, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("errors", doc["error"], "\ntolerance", doc["tolerance"], "\noracle vs mpmath", doc["oracle_vs_mpmath"],
          "\noracle vs log-space", doc["oracle_vs_logspace"], "\n%s: %d bytes" % (E.NPZ, os.path.getsize(E.NPZ)))


if __name__ == "__main__":
    main()
