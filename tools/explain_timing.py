#!/usr/bin/env python3
"""Kernel time of frisk_explain_ranges (csrc/explain_kernels.h) beside frisk_score_ranges on the same rows: the workloads of
tools/ranges_timing.py - a synthetic 64 Mb batch (16 scaffolds of 4 Mb, Engine.synth), k = 1..8, against its own profile:
  grid    every candidate window of w = 5000, i = 1000 passed as ranges
  mixed   50 000 ranges with seeded log-uniform lengths between 300 and 30 000 bases
  long    16 ranges of 4 Mb (the scaffolds themselves: the global-scratch form)
at top_n = 1, 16 and 64.  Each figure is frisk_last_kernel_ms (4: score, 7: explain), the median of --repeats calls after one
warm-up.  Prints one JSON line per workload and a markdown table.

    python tools/explain_timing.py [--repeats 3] [--device 0]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

from ranges_timing import median_ms  # noqa: E402

TOPS = (1, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scaffolds", type=int, default=16)
    ap.add_argument("--scaffold-len", type=int, default=4000000)
    a = ap.parse_args()
    from frisk_amd.engine import Engine
    lens = [a.scaffold_len] * a.scaffolds
    w, inc = 5000, 1000
    rows = []
    with Engine(1, 8, device=a.device) as e:
        e.synth(lens, 7, island_frac=0.02, n_frac=0.01, lower_frac=0.05)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        scan = e.scan(w, inc)
        jump = (scan.status & 4) != 0
        grid = (scan.seq_index.copy(), np.where(jump, scan.start, scan.start - 1), scan.stop.copy())
        rng = np.random.default_rng(11)
        n = 50000
        ln = np.exp(rng.uniform(np.log(300), np.log(30000), n)).astype(np.int64)
        s = rng.integers(0, len(lens), n).astype(np.int32)
        a0 = (rng.random(n) * (a.scaffold_len - ln)).astype(np.int64)
        mixed = (s, a0, a0 + ln)
        whole = (np.arange(len(lens), dtype=np.int32), np.zeros(len(lens), np.int64), np.asarray(lens, np.int64))
        for label, (si, st, sp) in (("grid", grid), ("mixed", mixed), ("long", whole)):
            score_ms = median_ms(lambda: e.score_ranges(si, st, sp), lambda: e.kernel_ms(4), a.repeats)
            res = {"workload": label, "ranges": int(si.size), "bases": int((sp - st).sum()), "score_kernel_ms": round(score_ms, 3)}
            for top_n in TOPS:
                ms = median_ms(lambda: e.explain_ranges(si, st, sp, top_n), lambda: e.kernel_ms(7), a.repeats)
                res["explain_kernel_ms_top%d" % top_n] = round(ms, 3)
                res["ratio_top%d" % top_n] = round(ms / score_ms, 2)
            got, ref = e.explain_ranges(si, st, sp, 1), e.score_ranges(si, st, sp)
            res["score_columns_agree"] = bool(all(getattr(got, c).tobytes() == getattr(ref, c).tobytes() for c in ("status", "kld", "gc", "nn")))
            print(json.dumps(res), flush=True)
            rows.append(res)
    print("| workload | ranges | score (ms) | " + " | ".join("explain top %d (ms) | ratio" % t for t in TOPS) + " |")
    print("|---|---|---|" + "---|---|" * len(TOPS))
    for r in rows:
        print("| %s | %d | %.2f | " % (r["workload"], r["ranges"], r["score_kernel_ms"]) +
              " | ".join("%.2f | %.2f" % (r["explain_kernel_ms_top%d" % t], r["ratio_top%d" % t]) for t in TOPS) + " |")


if __name__ == "__main__":
    main()
