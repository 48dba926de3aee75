#!/usr/bin/env python3
"""Kernel time of frisk_refine_ranges (csrc/refine_kernels.h) on the synthetic 64 Mb batch of tools/ranges_timing.py (16 scaffolds
of 4 Mb, Engine.synth), k = 1..8, against its own profile, on that tool's `mixed` workload: 50 000 ranges with seeded log-uniform
lengths between 300 and 30 000 bases, at flank 500 and 2000 and the default order, beside frisk_score_ranges on the same ranges.
Each figure is frisk_last_kernel_ms, the median of --repeats calls after one warm-up.  Prints one JSON line per run and a markdown
table.

    python tools/refine_timing.py [--repeats 3] [--device 0] [--orders 2 7]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

import region_workloads as RW  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    RW.add_arguments(ap)
    ap.add_argument("--orders", type=int, nargs="+", default=None, help="orders of the chains (default: the command line's default)")
    a = ap.parse_args()
    from frisk_amd import refine
    from frisk_amd.engine import Engine
    lens = [a.scaffold_len] * a.scaffolds
    orders = a.orders or [refine.default_order(1, 8)]
    rows = []
    with Engine(1, 8, device=a.device) as e:
        RW.synth_batch(e, lens)
        RW.own_profile(e)
        si, st, sp = RW.mixed(len(lens), a.scaffold_len)
        score_ms = RW.median_ms(lambda: e.score_ranges(si, st, sp), lambda: e.kernel_ms(4), a.repeats)
        for order in orders:
            for flank in (500, 2000):
                ms = RW.median_ms(lambda: e.refine_ranges(si, st, sp, flank, order), lambda: e.kernel_ms(8), a.repeats)
                got = e.refine_ranges(si, st, sp, flank, order)
                res = {"workload": "mixed", "ranges": int(si.size), "flank": flank, "order": order, "kernel_ms": round(ms, 3),
                       "ranges_per_s": round(si.size / (ms * 1e-3), 1), "score_ranges_kernel_ms": round(score_ms, 3),
                       "bases_searched": int(4 * got.flank_used.sum()), "moved": int(((got.new_start != st) | (got.new_stop != sp)).sum())}
                print(json.dumps(res), flush=True)
                rows.append(res)
    print("| order | flank | ranges | bases searched | kernel time (ms) | ranges/s |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %d | %d | %d | %.2f | %.0f |" % (r["order"], r["flank"], r["ranges"], r["bases_searched"], r["kernel_ms"], r["ranges_per_s"]))
    print("frisk_score_ranges, the same %d ranges: %.2f ms" % (rows[0]["ranges"], rows[0]["score_ranges_kernel_ms"]))


if __name__ == "__main__":
    main()
