#!/usr/bin/env python3
"""tests/golden/tsne_hp.json and tests/golden/tsne_hp/*.npy: the measured tolerances and recorded values of the extended-precision
t-SNE tests.

For every case of tests/tsne_hp_cases.py the float64 model (tests/tsne_oracle.py, direct differences) is compared with the
long-double oracle of tests/tsne_oracle_hp.py, as |model - oracle| / unit per entry.  Recorded: the SHA-256 of every input, the
bisection margins, the ratios per case, the worst per quantity, the allowed ratio = 8 x that worst, the ratio a Gram-form float64
evaluation reaches on the offset case, the oracle's own distance from 50-digit mpmath on three small cases, and what the tests
never recompute: beta, tries and margins of the n = 8192 / 8193 / 2049 cases, q and its unit on six rows of the first two, and S of
the centring case (with the ratio a float64 centring reaches in that case's own unit).  Nothing here comes from
the device, and this script does not use the package under test.

    python tools/make_golden_tsne_hp.py [--keep-recorded]       (the recorded arrays take several minutes; --keep-recorded
                                                                 reuses the files that are there)
"""
import json
import os
import sys
from multiprocessing import Pool

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import tsne_hp_cases as K  # noqa: E402
import tsne_oracle as TO  # noqa: E402
import tsne_oracle_hp as HP  # noqa: E402

LD = HP.LD


def _bisect_chunk(a):
    rid, i0 = a
    n, f, seed = K.RECORDED[rid]
    x = HP._ld(K.blobs(n, f, seed))
    return HP._bisect(x, np.arange(i0, min(n, i0 + HP.CHUNK)), LD(np.log(np.float64(K.perplexity_of(n)))))


def record(rid, keep):
    """beta, tries and margins of all rows (and q, u_q on the sampled rows of the two large cases) into tests/golden/tsne_hp."""
    n, f, seed = K.RECORDED[rid]
    X = K.blobs(n, f, seed)
    rows_file = os.path.join(K.DIR, rid + "_rows.npy")
    if not (keep and os.path.exists(rows_file)):
        with Pool(min(8, os.cpu_count() or 1)) as pool:
            parts = pool.map(_bisect_chunk, [(rid, i0) for i0 in range(0, n, HP.CHUNK)])
        np.save(rows_file, np.column_stack([np.concatenate([p[k] for p in parts]).astype(np.float64) for k in range(4)]))
    beta, tries, m_tol, m_sign = K.recorded_arrays(rid)
    _sumP, _r, total, rel_total = HP._totals(HP._ld(X), beta, f)
    doc = {"n": n, "f": f, "seed": seed, "X": K.sha(X), "perplexity": K.perplexity_of(n), "m_tol": float(m_tol.min()),
           "m_sign": float(m_sign.min()), "max_tries": int(tries.max()), "total": K.pair(total), "rel_total": K.pair(rel_total),
           "rows_sha": K.sha(np.load(rows_file))}
    if n > 8000:
        rows = K.SAMPLED_ROWS(n)
        o = HP.affinities(X, beta=beta, total=total, rel_total=rel_total, rows=rows)
        q = o["q"].astype(np.float64)
        # the unit as float32, rounded up, and widened by the rounding of q to float64 (half an ulp)
        uq = ((o["u_q"] + np.abs(q.astype(LD) - o["q"])) * (1 + LD(2.0) ** -20)).astype(np.float32)
        np.save(os.path.join(K.DIR, rid + "_q.npy"), q)
        np.save(os.path.join(K.DIR, rid + "_uq.npy"), uq)
        doc.update(sampled_rows=rows, q_sha=K.sha(q), uq_sha=K.sha(uq))
    return doc


def centring():
    X, Y0, perplexity = K.centre_inputs()
    y = HP._ld(Y0)
    n, d = y.shape
    S, hs = LD(0), LD(0)
    for i0 in range(0, n, HP.CHUNK):
        rr = np.arange(i0, min(n, i0 + HP.CHUNK))
        D, _ = HP._sqdist(y, rr)
        num = 1 / (1 + D)
        num[np.arange(len(rr)), rr] = 0
        S = S + HP._sum(HP._rowsum(num))
        hs = hs + HP._sum(HP._rowsum(num * (HP.EPS * ((d + 2) * D * num + 2))))
    return {"n": n, "d": d, "perplexity": perplexity, "X": K.sha(X), "Y0": K.sha(Y0), "rows": K.CENTRE_ROWS, "S": K.pair(S),
            "rel_S": K.pair(HP.EPS + hs / S), "model_ratio": K.centre_model(), "allowed": K.FACTOR * K.centre_model()}


def main():
    keep = "--keep-recorded" in sys.argv[1:]
    os.makedirs(K.DIR, exist_ok=True)
    doc = {"factor": K.FACTOR, "margin": K.MARGIN, "unit_eps": 2.0 ** -52, "quantities": list(K.QUANTITIES),
           "model": "tests/tsne_oracle.py: affinities and step(gram=False), float64 numpy, direct differences"}
    doc["recorded"] = {rid: record(rid, keep) for rid in sorted(K.RECORDED)}
    K.RECORDED_TOTALS.update(doc["recorded"])       # the step cases below take the recorded totals from here, not from the file
    aff = {}
    for c in K.AFF:
        o = K.oracle_aff(c)
        X = c.X()
        q = TO.affinities(X, c.perplexity)[2]
        m_tol, m_sign = K.margins(c, o)
        aff[c.id] = {"seed": c.seed, "X": K.sha(X), "perplexity": c.perplexity, "cap": c.cap, "m_tol": m_tol, "m_sign": m_sign,
                     "tries_50": int((o["tries"] == 50).sum()), "q": HP.ratio(q, o["q"], o["u_q"])}
        if c.kind == "offset":
            doc["gram_on_offset"] = {"case": c.id, "q": HP.ratio(K.gram_q(X, o["beta"]), o["q"], o["u_q"])}
    steps, kept = {}, {}
    for c in K.STEPS:
        r, st, m = K.model_step(c)
        Y, iY, gains = c.state(K.step_aff(c)["q"])
        steps[c.id] = {"X": K.sha(c.X()), "Y": K.sha(Y), "iY": K.sha(iY), "gains": K.sha(gains), "ratios": r,
                       "Q_clamped": st["Q_clamped"]}
        kept[c.id] = (st, m)
    worst = {"q": max([v["q"] for v in aff.values()] + [v["ratios"]["q"] for v in steps.values()]),
             "dY": max(v["ratios"]["dY"] for v in steps.values())}
    for c in K.STEPS:
        st, m = kept[c.id]
        r = K.compare_step(c, st, m.Y, m.iY, m.gains, m.cost, K.FACTOR * worst["dY"])
        steps[c.id]["ratios"].update({k: r[k] for k in ("iY", "Y", "cost") if k in r})
        steps[c.id]["undecided"] = int(K.undecided(st, K.FACTOR * worst["dY"]).sum())
        steps[c.id]["entries"] = int(m.Y.size)
    for k in ("iY", "Y", "cost"):
        worst[k] = max(v["ratios"].get(k, 0.0) for v in steps.values())
    doc.update(worst=worst, allowed={k: K.FACTOR * worst[k] for k in K.QUANTITIES}, affinity=aff, steps=steps,
               centring=centring(), oracle_vs_mpmath=K.mp_distances())
    with open(K.JSON, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("worst", worst)
    print("allowed", doc["allowed"])
    print("gram_on_offset", doc["gram_on_offset"])
    print("oracle_vs_mpmath", doc["oracle_vs_mpmath"])
    print("recorded", {k: (v["m_tol"], v["m_sign"]) for k, v in doc["recorded"].items()})


if __name__ == "__main__":
    main()
