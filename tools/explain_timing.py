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

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

import region_workloads as RW  # noqa: E402

TOPS = (1, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    RW.add_arguments(ap)
    a = ap.parse_args()
    from frisk_amd.engine import Engine
    lens = [a.scaffold_len] * a.scaffolds
    w, inc = RW.W, RW.INC
    rows = []
    with Engine(1, 8, device=a.device) as e:
        RW.synth_batch(e, lens)
        RW.own_profile(e)
        workloads = (("grid", RW.grid_of(e.scan(w, inc))), ("mixed", RW.mixed(len(lens), a.scaffold_len)), ("long", RW.whole(lens)))
        for label, (si, st, sp) in workloads:
            score_ms = RW.median_ms(lambda: e.score_ranges(si, st, sp), lambda: e.kernel_ms(4), a.repeats)
            res = {"workload": label, "ranges": int(si.size), "bases": int((sp - st).sum()), "score_kernel_ms": round(score_ms, 3)}
            for top_n in TOPS:
                ms = RW.median_ms(lambda: e.explain_ranges(si, st, sp, top_n), lambda: e.kernel_ms(7), a.repeats)
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
