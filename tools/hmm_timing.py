#!/usr/bin/env python3
"""Wall-clock of the 2-state HMM at the row counts of a GRCh38-sized run: host-native (csrc/hmm_host.h) against the device form
(csrc/hmm_kernels.h), fit and Viterbi, at n = 3.06 M (the default -w 5000 -i 2500 table's order) and 6.6 M (--updateHMM's fine
pass, -w 1000 -i 500).  Host arrays in and out on both sides: the device figures include the upload of the scores, the
allocations and the download of the states - what a caller of GaussianHMM2(native="gpu") waits for.  Each figure is the median
of --repeats runs after one warm-up; prints one JSON line per size and a markdown table.

    python tools/hmm_timing.py [--sizes 3060000 6600000] [--repeats 3] [--device 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))


def track(n, seed=11, scaffold=250000):
    """KLD-like scores: two regimes, and scaffolds of `scaffold` windows (a human chromosome is ~500 k fine windows)."""
    rng = np.random.default_rng(seed)
    st = np.cumsum(rng.random(n) < 0.002) % 2
    x = np.where(st == 0, rng.normal(0.03, 0.01, n), rng.normal(0.12, 0.05, n)).clip(1e-4, None)
    off = np.unique(np.concatenate((np.arange(0, n, scaffold), [n]))).astype(np.int64)
    return np.ascontiguousarray(x), off


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[3060000, 6600000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from frisk_amd.hmm import GaussianHMM2
    rows = []
    for n in a.sizes:
        x, off = track(n)
        res = {"n": n, "segments": int(off.size - 1)}
        models = {}
        for label, native in (("host", True), ("device", "gpu")):
            m = GaussianHMM2(native=native, device=a.device)
            res[label + "_fit_s"] = timed(lambda m=m: m.fit(x), a.repeats)
            res[label + "_viterbi_s"] = timed(lambda m=m: m.predict_segments(x, off), a.repeats)
            res[label + "_rounds"] = m.n_iter_
            models[label] = (m, m.predict_segments(x, off))
        h, d = models["host"], models["device"]
        res["states_differ"] = int(np.count_nonzero(h[1] != d[1]))
        res["max_param_diff"] = float(max(np.max(np.abs(np.ravel(getattr(h[0], f)) - np.ravel(getattr(d[0], f))))
                                          for f in ("means_", "covars_", "startprob_", "transmat_")))
        print(json.dumps(res), flush=True)
        rows.append(res)
    print("| rows | fit host-native (s) | fit device (s) | Viterbi host-native (s) | Viterbi device (s) |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.3f | %.3f | %.3f | %.3f |" % (r["n"], r["host_fit_s"], r["device_fit_s"], r["host_viterbi_s"], r["device_viterbi_s"]))


if __name__ == "__main__":
    main()
