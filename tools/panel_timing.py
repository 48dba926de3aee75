#!/usr/bin/env python3
"""Kernel time of frisk_score_ranges_panel (csrc/panel_kernels.h) beside P calls of frisk_score_ranges (csrc/range_kernels.h), on
the synthetic batch of tools/ranges_timing.py (16 scaffolds of 4 Mb, Engine.synth seed 7), k = 1..8, and its two short-form
workloads:
  grid    every candidate window of w = 5000, i = 1000 passed as ranges
  mixed   50 000 ranges with seeded log-uniform lengths between 300 and 30 000 bases
For P in 1, 4, 16 profiles - each the profile of a synthetic genome of its own seed, pushed to the panel -:
  (a) panel    frisk_last_kernel_ms(ctx, 5) of one panel call
  (b) single   the sum of frisk_last_kernel_ms(ctx, 4) over P calls of frisk_score_ranges, with profile_set between them
Each figure is the median of --repeats measurements after one warm-up.  Prints one JSON line per workload and P, and a markdown
table.

    python tools/panel_timing.py [--repeats 3] [--device 0]
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
    ap.add_argument("--profiles", type=int, nargs="+", default=[1, 4, 16])
    a = ap.parse_args()
    from frisk_amd.engine import Engine
    lens = [a.scaffold_len] * a.scaffolds
    w, inc = RW.W, RW.INC
    rows = []
    with Engine(1, 8, device=a.device) as e:
        profs = []
        for p in range(max(a.profiles)):                # donor p: a synthetic genome of its own
            RW.synth_batch(e, lens, seed=100 + p)
            RW.own_profile(e)
            profs.append(e.profile_get())
        RW.synth_batch(e, lens)
        e.profile_set(*profs[0])
        workloads = (("grid", RW.grid_of(e.scan(w, inc))), ("mixed", RW.mixed(len(lens), a.scaffold_len)))
        for P in a.profiles:
            e.panel_reset()
            for prof in profs[:P]:
                e.profile_set(*prof)
                e.panel_push()
            for label, (si, st, sp) in workloads:
                def panel():
                    e.score_ranges_panel(si, st, sp)
                    return e.kernel_ms(5)

                def single():
                    total = 0.0
                    for prof in profs[:P]:
                        e.profile_set(*prof)
                        e.score_ranges(si, st, sp)
                        total += e.kernel_ms(4)
                    return total
                pa, sg = RW.median_ms(panel, None, a.repeats), RW.median_ms(single, None, a.repeats)
                got, one = e.score_ranges_panel(si, st, sp), e.score_ranges(si, st, sp)     # (the context holds profile P - 1)
                res = {"workload": label, "profiles": P, "ranges": int(si.size), "bases": int((sp - st).sum()),
                       "panel_ms": round(pa, 3), "single_ms_sum": round(sg, 3), "panel_over_single": round(pa / sg, 3),
                       "last_plane_bit_equal": bool(got.kld[P - 1].tobytes() == one.kld.tobytes() and
                                                    got.status[P - 1].tobytes() == one.status.tobytes())}
                print(json.dumps(res), flush=True)
                rows.append(res)
    print("| workload | ranges | P | (a) one panel call (ms) | (b) P single-profile calls (ms) | (a) / (b) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.2f | %.2f | %.2f |" % (r["workload"], r["ranges"], r["profiles"], r["panel_ms"], r["single_ms_sum"],
                                                        r["panel_over_single"]))


if __name__ == "__main__":
    main()
