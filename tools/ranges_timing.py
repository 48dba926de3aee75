#!/usr/bin/env python3
"""Kernel time of frisk_score_ranges (csrc/range_kernels.h) on a synthetic 64 Mb batch (16 scaffolds of 4 Mb, Engine.synth),
k = 1..8, against its own profile:
  grid    every candidate window of w = 5000, i = 1000 passed as ranges, beside frisk_scan's kernel time for the same windows
  mixed   50 000 ranges with seeded log-uniform lengths between 300 and 30 000 bases
  long    16 ranges of 4 Mb (the scaffolds themselves: the global-scratch form)
Each figure is frisk_last_kernel_ms, the median of --repeats calls after one warm-up.  Prints one JSON line per workload and a
markdown table.

    python tools/ranges_timing.py [--repeats 3] [--device 0]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

import region_workloads as RW  # noqa: E402


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
        scan = e.scan(w, inc)
        scan_ms = RW.median_ms(lambda: e.scan(w, inc, pinned=True), lambda: e.kernel_ms(0), a.repeats)
        workloads = (("grid", RW.grid_of(scan)), ("mixed", RW.mixed(len(lens), a.scaffold_len)), ("long", RW.whole(lens)))
        for label, (si, st, sp) in workloads:
            ms = RW.median_ms(lambda: e.score_ranges(si, st, sp), lambda: e.kernel_ms(4), a.repeats)
            res = {"workload": label, "ranges": int(si.size), "bases": int((sp - st).sum()), "kernel_ms": round(ms, 3),
                   "ranges_per_s": round(si.size / (ms * 1e-3), 1)}
            if label == "grid":
                res["scan_kernel_ms"] = round(scan_ms, 3)
                res["ratio_to_scan"] = round(ms / scan_ms, 2)
                got = e.score_ranges(si, st, sp)
                res["status_agrees_with_scan"] = bool(np.array_equal(scan.status & ~np.uint32(4), got.status))
            print(json.dumps(res), flush=True)
            rows.append(res)
    print("| workload | ranges | bases | kernel time (ms) | ranges/s |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.2f | %.0f |" % (r["workload"], r["ranges"], r["bases"], r["kernel_ms"], r["ranges_per_s"]))
    print("frisk_scan, the same %d windows: %.2f ms (ranges / scan = %.2f)" % (rows[0]["ranges"], rows[0]["scan_kernel_ms"],
                                                                             rows[0]["ratio_to_scan"]))


if __name__ == "__main__":
    main()
