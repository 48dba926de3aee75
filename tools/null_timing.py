#!/usr/bin/env python3
"""Time of the length-matched nulls (HotPath.nullScores) on the synthetic batch of tools/ranges_timing.py (16 scaffolds of 4 Mb,
Engine.synth, 1 % N, 5 % soft-masked), k = 1..8, against its own profile: 10 000 regions of seeded log-uniform lengths between
300 and 30 000 bases, 100 draws per distinct length, both nulls.
  generator   frisk_last_kernel_ms(ctx, 6): the table and draw kernels of frisk_seq_null (markov only)
  scoring     frisk_last_kernel_ms(ctx, 4), summed over the score_ranges calls of one nullScores
  wall        the whole nullScores call, host side included
Each figure is the median of --repeats calls after one warm-up.  Prints one JSON line per null and a markdown table (DESIGN.md
section 15).

    python tools/null_timing.py [--repeats 3] [--device 0]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

import region_workloads as RW  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    RW.add_arguments(ap)
    ap.add_argument("--regions", type=int, default=10000)
    ap.add_argument("--draws", type=int, default=100)
    a = ap.parse_args()
    from frisk_amd.hotpath import HotPath
    lens = [a.scaffold_len] * a.scaffolds
    rng = np.random.default_rng(11)
    lengths = sorted({int(x) for x in RW.log_uniform_lengths(rng, a.regions)})
    hp = HotPath(1, 8, device=a.device)
    e = hp.engine
    rows = []
    try:
        RW.synth_batch(e, lens)
        RW.own_profile(e)
        hp._resident, hp.names = "synthetic", [""] * len(lens)         # (the host null scores the resident batch as the host)
        args = SimpleNamespace(hostSeq="synthetic")
        scored = {"ms": 0.0}
        real = e.score_ranges

        def timed(*p, **k):
            res = real(*p, **k)
            scored["ms"] += e.kernel_ms(4)
            return res
        e.score_ranges = timed
        for mode in ("host", "markov"):
            gen, score, wall, valid = [], [], [], 0
            for it in range(a.repeats + 1):
                scored["ms"] = 0.0
                t0 = time.perf_counter()
                kld, ok = hp.nullScores(args, lengths, a.draws, 5, mode)
                t1 = time.perf_counter()
                if it:
                    gen.append(e.kernel_ms(6)); score.append(scored["ms"]); wall.append((t1 - t0) * 1e3)
                valid = int(ok.sum())
            res = {"null": mode, "regions": a.regions, "lengths": len(lengths), "draws": a.draws, "ranges": len(lengths) * a.draws,
                   "valid": valid, "bases_scored": int(sum(lengths)) * a.draws,
                   "generator_ms": round(statistics.median(gen), 3) if mode == "markov" else None,
                   "scoring_ms": round(statistics.median(score), 3), "wall_ms": round(statistics.median(wall), 1)}
            print(json.dumps(res), flush=True)
            rows.append(res)
    finally:
        hp.close()
    print("| null | distinct lengths | ranges scored | valid | generator (ms) | scoring kernels (ms) | nullScores, wall (ms) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %d | %s | %.2f | %.0f |" % (r["null"], r["lengths"], r["ranges"], r["valid"],
                                                          "-" if r["generator_ms"] is None else "%.3f" % r["generator_ms"],
                                                          r["scoring_ms"], r["wall_ms"]))


if __name__ == "__main__":
    main()
