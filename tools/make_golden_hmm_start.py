#!/usr/bin/env python3
"""Golden data of the tests of the HMM's deterministic start and first EM rounds (tests/hmm_start_cases.py): everything here is
measured on the CPU, nothing on a GPU.

tests/golden/hmm_start.json holds, for every case: the input's sha256, the oracle's 2-means round count, the error against the
long-double oracle (tests/hmm_oracle_hp.py) of three float64 forms - the numpy specification, the float64 model in the device's
layout (tests/hmm_start_model.py) and the host-native library -, the oracle's own distance from 50-digit mpmath where the case is
small enough, and for the large sizes the oracle's values as (high, low) pairs of doubles.  The tolerance of a quantity is FACTOR x
the largest of those errors over the whole case set.  Every input is first held to the conditions of hmm_start_cases (assignment
margin, stop-rule margin, log-likelihood gap): a case that fails stops the run and wants another seed (hmm_start_cases.RESEED).

    python tools/make_golden_hmm_start.py [--jobs 8]
"""
import argparse
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import hmm_estep_cases as E  # noqa: E402
import hmm_gpu_cases as H  # noqa: E402
import hmm_oracle_hp as O  # noqa: E402
import hmm_start_cases as S  # noqa: E402
import hmm_start_model as SM  # noqa: E402

MP_START, MP_ROUNDS = 257, 129      # mpmath runs on the cases of at most this many windows


def start_one(case):
    family, n = case
    x = S.start_input(family, n)
    st = O.start(x, S.MIN_COVAR)
    S.start_conditions(family, n, st)
    ref = S.ref_of_start(st)
    out = {"n": n, "sha256": H.sha(x), "rounds": ref["rounds"], "error": {}}
    means, covar, rounds = SM.start(x, "device")
    assert rounds == ref["rounds"]
    out["error"]["model"] = S.start_errors((means, [covar, covar]), ref)
    for form, native in (("numpy", False), ("host", True)):
        out["error"][form] = S.start_errors(S.fit_start(x, native)[1], ref)
    if n <= MP_START:
        out["oracle_vs_mpmath"] = dict(zip(S.START_Q, O.start_distance_from_mp(x, S.MIN_COVAR)))
    if n in S.LARGE:
        out["oracle"] = S.pack_start(ref)
    print("%-22s rounds %3d  %s" % (S.start_id(*case), ref["rounds"], "  ".join(
        "%s %.2g %.2g" % ((f,) + tuple(out["error"][f][q] for q in S.START_Q)) for f in S.FORMS)), flush=True)
    return "start", S.start_id(*case), out


def round_one(case):
    family, n = case
    x = S.round_input(family, n)
    fr = O.fit_rounds(x, max(S.ROUNDS), S.MIN_COVAR, S.COVARS_PRIOR)
    S.round_conditions(family, n, [ll for _m, ll in fr])
    ref = S.ref_of_rounds(fr)
    out = {"n": n, "sha256": H.sha(x), "error": {f: {} for f in S.FORMS}}
    model, spec = SM.fit(x, max(S.ROUNDS)), S.numpy_rounds(x)
    for r in S.ROUNDS:
        out["error"]["model"].update(S.round_errors(r, model[r - 1], ref))
        out["error"]["numpy"].update(S.round_errors(r, spec[r], ref))
        out["error"]["host"].update(S.round_errors(r, S.fit_rounds(x, r, True)[1], ref))
    if n <= MP_ROUNDS:
        d = O.rounds_distance_from_mp(x, S.ROUNDS, S.MIN_COVAR, S.COVARS_PRIOR)
        out["oracle_vs_mpmath"] = {"fit%d_%s" % (r, k): d[r][i] for r in S.ROUNDS for i, k in enumerate(("params", "loglik"))}
    if n in E.LARGE:
        out["oracle"] = S.pack_rounds(ref)
    print("%-24s %s" % (S.round_id(*case), "  ".join(
        "%s %s" % (f, " ".join("%.2g" % out["error"][f][q] for q in S.ROUND_Q)) for f in S.FORMS)), flush=True)
    return "round", S.round_id(*case), out


def one(task):
    return (start_one if task[0] == "start" else round_one)(task[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    tasks = ([("round", c) for c in S.round_cases(E.LARGE[::-1])] + [("start", c) for c in S.start_cases(S.LARGE[::-1])]      # (the slow ones first)
             + [("round", c) for c in S.round_cases(E.SMALL[::-1])] + [("start", c) for c in S.start_cases(S.SMALL[::-1])])
    with multiprocessing.Pool(a.jobs) as pool:
        results = pool.map(one, tasks, chunksize=1)
    doc = {"factor": S.FACTOR, "oracle_margin": S.ORACLE_MARGIN, "margin": H.MARGIN, "stop_margin": S.STOP_MARGIN, "gap": H.GAP,
           "sizes": list(S.SIZES), "large": list(S.LARGE), "round_sizes": list(S.ROUND_SIZES), "round_model": S.ROUND_MODEL,
           "start_cases": {}, "round_cases": {}}
    for kind, cid, out in sorted(results, key=lambda r: r[:2]):
        doc["start_cases" if kind == "start" else "round_cases"][cid] = out
    cases_of = lambda q: doc["start_cases" if q in S.START_Q else "round_cases"].values()      # noqa: E731
    doc["error"] = {f: {q: max(c["error"][f][q] for c in cases_of(q)) for q in S.QUANTITIES} for f in S.FORMS}
    doc["oracle_vs_mpmath"] = {q: max(c["oracle_vs_mpmath"][q] for c in cases_of(q) if "oracle_vs_mpmath" in c) for q in S.QUANTITIES}
    doc["tolerance"] = {q: S.FACTOR * max(doc["error"][f][q] for f in S.FORMS) for q in S.QUANTITIES}
    # the numpy specification works in log space, whose absolute error grows with n: it sets the round tolerances (1e-8 at 524288
    # windows).  The two forms that work in scaled space, as the device does, give a second, tighter bound of the same making
    doc["tolerance_scaled_forms"] = {q: S.FACTOR * max(doc["error"][f][q] for f in ("model", "host")) for q in S.QUANTITIES}
    for q in S.QUANTITIES:
        assert S.ORACLE_MARGIN * doc["oracle_vs_mpmath"][q] <= doc["tolerance_scaled_forms"][q], q
    doc["max_rounds_up_to_4096"] =max(c["rounds"] for c in doc["start_cases"].values() if c["n"] <= 4096)
    for q in S.QUANTITIES:
        assert S.ORACLE_MARGIN * doc["oracle_vs_mpmath"][q] <= doc["tolerance"][q], (q, doc["oracle_vs_mpmath"], doc["tolerance"])
    with open(S.JSON, "w") as fh:
        json.dump(doc, fh, indent=0)
    print("errors", json.dumps(doc["error"], indent=1), "\ntolerance", doc["tolerance"], "\ntolerance from the scaled-space forms", doc["tolerance_scaled_forms"], "\noracle vs mpmath", doc["oracle_vs_mpmath"],
          "\nmost 2-means rounds at n <= 4096: %d" % doc["max_rounds_up_to_4096"], "\n%s: %d bytes" % (S.JSON, os.path.getsize(S.JSON)))


if __name__ == "__main__":
    main()
