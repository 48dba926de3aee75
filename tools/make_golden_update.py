#!/usr/bin/env python3
"""Golden data of --updateHMM (data only; nothing of the reference is copied into this repository).

1. tests/golden/update_hmm.json: the reference's OWN updateHMM (frisk/__init__.py L737-755; marked "not currently in use" there)
   run on hand-made and generated cases.  The reference module is loaded the way tools/make_golden.py loads it (lib2to3 in a
   scratch directory, only the named FunctionDefs exec'd), with the same pybedtools stand-in: updateHMM hands its result to
   pybedtools.BedTool, and the stand-in keeps the records as they were given.
2. tests/golden/hmm_gpu.json: what qualifies the inputs of the device-HMM tests (tests/hmm_gpu_cases.py) - for every fit case the
   sha256 of the regenerated input, the numpy specification's fit (minutes on the 3 M-row case, which is why it is recorded), the
   spread between the numpy specification and the host-native fit, and the distance of every round's log-likelihood gain from
   tol; for every Viterbi case the sha256 of input and numpy states and the smallest decision margin of the numpy path.  The
   device tolerance is FACTOR x the largest spread: both numbers are written.

    python tools/make_golden_update.py [--only update|hmm|viterbi]      (viterbi: refresh the Viterbi cases of hmm_gpu.json alone)
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden as MG  # noqa: E402


def update_cases():
    from frisk_amd.hmm import hmm2BED
    cases = []

    def add(name, fine, anomalies):
        cases.append({"name": name, "fine": [list(map(str, r)) for r in fine], "anomalies": [list(map(str, r)) for r in anomalies]})

    add("ties_at_equal_distance",
        [("s1", 1, 1000, "State1"), ("s1", 501, 1400, "State2"), ("s1", 901, 2000, "State1")],
        # 1200 is 200 from 1000 and from 1400, 1700 is 300 from 1400 and from 2000: the first in list order wins; 951 is 50 / 49 from 901 / 1000
        [("s1", 750, 1200, "0.5"), ("s1", 700, 1700, "0.4"), ("s1", 951, 1450, "0.3"), ("s1", 1, 1, "0.2")])
    add("boundary_on_an_anomaly_edge",
        [("s1", 1, 5000, "State1"), ("s1", 4001, 9000, "State2"), ("s1", 8001, 12000, "State1")],
        [("s1", 4001, 9000, "0.9"), ("s1", 5000, 8001, "0.8"), ("s1", 1, 12000, "0.7"), ("s1", 4500, 4500, "0.6")])
    add("several_scaffolds",
        [("chr2", 1, 3000, "State1"), ("chr10", 1, 2000, "State2"), ("chr2", 2501, 7000, "State2"), ("chr10", 1501, 6000, "State1"),
         ("chrX", 1, 1000, "State1")],
        [("chr10", 1400, 5000, "0.5"), ("chr2", 2600, 6500, "0.4"), ("chrX", 400, 800, "0.3"), ("chr2", 1, 2400, "0.2")])
    # string-sorted interval order and single-window states: what hmm2BED itself emits (starts compare as text: '10001' < '2001')
    rng = np.random.default_rng(7)
    rows = []
    for name, n in (("chr2", 60), ("chr10", 45)):
        st = np.cumsum(rng.random(n) < 0.15) % 2
        k = np.where(st == 0, rng.normal(0.03, 0.004, n), rng.normal(0.12, 0.01, n))
        k[7] = 0.12 if st[7] == 0 else 0.03             # a single window of the other state
        rows += [(name, 1 + 500 * i, 1000 + 500 * i, float(v), 0.5) for i, v in enumerate(k)]
    fine, _model = hmm2BED(rows)
    assert fine == sorted(fine, key=lambda t: (t[0], t[1], t[2])) and any(int(f[2]) - int(f[1]) == 999 for f in fine)
    assert [int(f[1]) for f in fine if f[0] == "chr2"] != sorted(int(f[1]) for f in fine if f[0] == "chr2")
    anomalies = [("chr2", 2300, 9100, "0.4"), ("chr2", 14800, 21700, "0.3"), ("chr10", 900, 4400, "0.5"), ("chr10", 20000, 23000, "0.2"),
                 ("chr2", 3501, 4500, "0.1")]
    add("string_sorted_order_and_single_windows", fine, anomalies)
    return cases


def run_update():
    ns = MG.load_reference_functions(extra=("updateHMM",))
    out = []
    for c in update_cases():
        got = ns["updateHMM"]([tuple(r) for r in c["fine"]], [tuple(r) for r in c["anomalies"]])
        c["expected"] = [list(r) for r in got]
        assert len(c["expected"]) == len(c["anomalies"])
        out.append(c)
    # the KeyError the CLI's first rule replaces
    try:
        ns["updateHMM"]([("s1", "1", "100", "State1")], [("s2", "1", "50")])
        raised = None
    except KeyError as err:
        raised = repr(err)
    doc = {"source": "reference updateHMM, frisk/__init__.py L737-755, through tools/make_golden_update.py", "cases": out,
           "missing_scaffold_raises": raised}
    with open(os.path.join(GOLD, "update_hmm.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    print("update_hmm.json: %d cases, missing scaffold -> %s" % (len(out), raised))


def run_hmm(viterbi_only=False):
    import hmm_gpu_cases as H
    import hmm_piece_model as PM
    from frisk_amd.hmm import GaussianHMM2
    doc = {"factor": H.FACTOR, "margin": H.MARGIN, "gap": H.GAP, "fit": {}, "viterbi": {}}
    if viterbi_only:                        # (the fit cases stand as recorded: the numpy fit of the 3 M rows takes minutes)
        doc = json.load(open(os.path.join(GOLD, "hmm_gpu.json")))
        doc["viterbi"] = {}
    worst = doc.get("spread_numpy_host", 0.0)
    for name in ([] if viterbi_only else H.FIT_CASES):
        x = H.fit_input(name)
        spec = H.RecordingHMM().fit(x)
        host = GaussianHMM2(native=True).fit(x)
        assert spec.n_iter_ == host.n_iter_, name
        sp = H.spread(H.params(spec), H.params(host), spec.loglik_, host.loglik_)
        gap_spec = H.gap_from_tol(spec.lls)
        gap_host = H.gap_from_tol(H.native_lls(x, host.n_iter_))
        assert min(gap_spec, gap_host) >= H.GAP, (name, gap_spec, gap_host)
        worst = max(worst, sp)
        doc["fit"][name] = {"n": int(x.size), "sha256": H.sha(x), "numpy": dict(H.params(spec), loglik_=spec.loglik_, n_iter_=spec.n_iter_),
                            "numpy_lls": spec.lls, "spread_numpy_host": sp, "gap_from_tol": min(gap_spec, gap_host)}
        print("fit %-14s n %8d rounds %2d spread %.3g gap %.3g" % (name, x.size, spec.n_iter_, sp, min(gap_spec, gap_host)), flush=True)
    doc["spread_numpy_host"] = worst
    doc["tolerance"] = H.FACTOR * worst
    for name in H.VITERBI_CASES:
        x, seg_off, model = H.viterbi_case(name)
        count = {}
        states, margin = H.numpy_states(model, x, seg_off, with_margin=True, count=count)
        if name in H.TIED:                  # exact ties everywhere: nothing to demand of the margin; all zeros, first on the piece model
            pm = np.concatenate([PM.viterbi(x[a:b], model) for a, b in zip(seg_off[:-1].tolist(), seg_off[1:].tolist())] + [[]])
            assert margin == 0.0 and not states.any() and not pm.any(), name
        else:
            assert margin > H.MARGIN, (name, margin)
        assert np.array_equal(states, H.numpy_states(model, x, seg_off)), name
        doc["viterbi"][name] = {"decisions": count, "n": int(x.size), "segments": int(seg_off.size - 1), "sha256": H.sha(x), "states_sha256": H.sha(states),
                                "margin": margin, "state1_fraction": float(states.mean()) if states.size else 0.0}
        print("viterbi %-15s n %7d margin %.3g" % (name, x.size, margin), flush=True)
    with open(os.path.join(GOLD, "hmm_gpu.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    print("hmm_gpu.json: spread %.3g, tolerance %.3g" % (worst, doc["tolerance"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["update", "hmm", "viterbi"], default=None)
    a = ap.parse_args()
    if a.only in (None, "update"):
        run_update()
    if a.only in (None, "hmm"):
        run_hmm()
    if a.only == "viterbi":
        run_hmm(viterbi_only=True)


if __name__ == "__main__":
    main()
