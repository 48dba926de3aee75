#!/usr/bin/env python3
"""Golden data and throughput figure of --gffIn (data only; nothing of the reference or of bedtools is run or copied).

1. tests/golden/bedtools_window_semantics.json: the cases below, each with the kept records written down BY HAND from the
   documented behaviour of `bedtools window` (`-w`: A widened by w on either side, the start clipped at 0; `-u`: an A record once
   if anything of B lies in the window; a GFF record's start shifted by one to BED numbers; B in BED numbers as given).  Before
   the file is written, every hand-written answer is checked against the overlap LENGTH of the two intervals,
   min(a_hi, b_end) - max(a_lo, b_start) > 0 - neither the sweep of frisk_amd.postprocess.window_u nor the pair of inequalities
   its docstring states.
2. --time: frisk_amd.postprocess.featuresNear on a synthetic annotation (default 3 M features, 10 000 regions, 24 chroms), and a
   pure-Python loop over every (feature, region) pair on a 1 % sample of the features as the yardstick.

    python tools/make_golden_gffin.py [--time [--features N] [--regions M]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

PROVENANCE = (
    "DATA, not output of a program: bedtools is absent from this image and there is no network, so these cases are transcribed "
    "by hand from the documented behaviour of `bedtools window` (manual page of window: `-w` = base pairs added upstream and "
    "downstream of each entry in A when searching for overlaps in B, the widened start clipped at 0; `-u` = write the original A "
    "entry once if any overlaps are found in B; overlap = at least one shared base in half-open BED arithmetic, so book-ended "
    "features do not overlap) and of bedtools' GFF reader (a GFF record's 1-based inclusive start is shifted by one, "
    "[start - 1, end); a BED record is taken as it is).  The reference calls `BedTool(gffIn).each(gffFilter, feature=TYPES)"
    ".window(b=REGIONS, w=gffRange, u=True)` (frisk/__init__.py L1714-1715, L1726-1733) with the anomalies as BED records "
    "carrying the score table's start / stop unchanged and the HMM states as GFF records.  `gff` holds the A file's lines, "
    "`feature_types` the list gffFilter tests column 3 against with Python's `in`, `regions` B in BED numbers, `expected` the "
    "kept lines in file order.  They pin frisk_amd.postprocess.read_gff / window_u / featuresNear to something other than "
    "themselves; tools/make_golden_gffin.py checks each answer against the overlap length of the intervals before writing.")


def g(chrom, kind, start, end, ident):
    return "\t".join([chrom, "hand", kind, str(start), str(end), ".", "+", ".", "ID=" + ident])


def cases():
    out = []

    def add(name, w, types, gff, regions, expected):
        out.append({"name": name, "w": w, "feature_types": types, "gff": gff, "regions": regions, "expected": expected})

    left, right = g("c1", "gene", 51, 100, "left"), g("c1", "gene", 201, 300, "right")
    add("book-ended on either side of a region, w = 0: not kept", 0, ["gene"], [left, right], [["c1", 100, 200]], [])
    add("book-ended on either side of a region, w = 1: kept", 1, ["gene"], [left, right], [["c1", 100, 200]], [left, right])
    one = [g("c1", "gene", 100, 100, "base100"), g("c1", "gene", 101, 101, "base101"), g("c1", "gene", 102, 102, "base102")]
    add("the GFF minus-one shift decides a one-base case: GFF 101..101 is BED [100, 101)", 0, ["gene"], one, [["c1", 100, 101]],
        [one[1]])
    near0 = [g("c1", "gene", 5, 10, "near0")]
    add("clipping at 0: [4 - 3, 10 + 3) = [1, 13) is book-ended with [0, 1)", 3, ["gene"], near0, [["c1", 0, 1]], [])
    add("clipping at 0: w = 50 gives [0, 60), not [-46, 60)", 50, ["gene"], near0 + [g("c1", "gene", 80, 90, "far")],
        [["c1", 0, 1], ["c1", 140, 150]], near0)
    mid = [g("c1", "gene", 221, 280, "mid")]
    add("a feature near two regions is reported once (-u)", 25, ["gene"], mid, [["c1", 100, 200], ["c1", 300, 400]], mid)
    add("a feature inside three overlapping regions is reported once (-u)", 0, ["gene"], mid,
        [["c1", 100, 400], ["c1", 200, 300], ["c1", 250, 260]], mid)
    two = [g("c1", "gene", 150, 160, "on_c1"), g("c2", "gene", 150, 160, "on_c2")]
    add("a region on another chrom does not count", 1000, ["gene"], two, [["c2", 100, 200]], [two[1]])
    three = [g("c3", "gene", 150, 160, "on_c3"), g("c1", "gene", 150, 160, "on_c1"), g("c3", "gene", 1, 5, "on_c3_too")]
    add("a chrom absent from B keeps nothing", 5, ["gene"], three, [["c1", 100, 200], ["c10", 100, 200]], [three[1]])
    nest = [g("c1", "gene", 951, 990, "under_the_long_one"), g("c1", "gene", 1001, 1100, "book_ended_with_the_long_one"),
            g("c1", "gene", 5050, 5060, "in_the_first_listed"), g("c2", "gene", 21, 30, "book_ended_on_c2"),
            g("c1", "gene", 50, 100, "before_all")]
    add("nested and unsorted B: the region that starts last before a feature need not be the one that reaches it", 0, ["gene"],
        nest, [["c1", 5000, 5100], ["c1", 100, 1000], ["c1", 200, 300], ["c2", 10, 20], ["c1", 900, 950]], [nest[0], nest[2]])
    kinds = [g("c1", "gene", 110, 190, "g1"), g("c1", "mRNA", 110, 190, "g1.t1"), g("c1", "exon", 110, 150, "g1.t1.e1"),
             g("c1", "CDS", 120, 150, "g1.t1.c1"), g("c1", "tRNA", 160, 180, "t1"), g("c1", "pseudogene", 130, 140, "p1"),
             g("c1", "gen", 130, 140, "not_a_substring_test"), g("c1", "gene", 400, 500, "g2")]
    add("a type filter with several types: list membership, in file order", 0, ["tRNA", "gene"], kinds, [["c1", 100, 200]],
        [kinds[0], kinds[4]])
    wide = [g("c1", "gene", 1, 10, "first_bases"), g("c1", "gene", 3990, 4000, "last_bases"), g("c2", "gene", 1, 10, "other")]
    add("w larger than the scaffold: everything on a chrom that has a region", 10 ** 9, ["gene"], wide, [["c1", 2000, 2001]],
        wide[:2])
    return out


def overlap_length_rule(case):
    """The kept lines by the overlap length of widened A and B - the check on the hand-written answers."""
    kept = []
    for line in case["gff"]:
        f = line.split("\t")
        if f[2] not in case["feature_types"]:
            continue
        a_lo, a_hi = max(0, int(f[3]) - 1 - case["w"]), int(f[4]) + case["w"]
        if any(r[0] == f[0] and min(a_hi, r[2]) - max(a_lo, r[1]) > 0 for r in case["regions"]):
            kept.append(line)
    return kept


def write_golden():
    doc = {"provenance": PROVENANCE, "cases": cases()}
    for c in doc["cases"]:
        assert overlap_length_rule(c) == c["expected"], c["name"]
    path = os.path.join(GOLD, "bedtools_window_semantics.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("%s: %d cases" % (path, len(doc["cases"])))


def brute_force(a_chrom, a_start, a_end, regions, w):
    """One Python step per (feature, region) pair."""
    mask = []
    for c, s, e in zip(a_chrom, a_start, a_end):
        lo, hi = max(0, s - w), e + w
        hit = False
        for rc, rs, re_ in regions:
            if rc == c and lo < re_ and rs < hi:
                hit = True
        mask.append(hit)
    return mask


def timing(n_feat, n_reg, w=1000, chroms=24, seed=5):
    from frisk_amd import postprocess as pp
    rng = np.random.default_rng(seed)
    length = 130_000_000
    names = np.asarray(["chr%d" % (i + 1) for i in range(chroms)], dtype=object)
    a_chrom = names[np.sort(rng.integers(0, chroms, n_feat))]
    a_start = rng.integers(0, length, n_feat)
    a_end = a_start + rng.integers(1, 20000, n_feat)
    recs = pp.GffRecords(["%s\tsynth\tgene\t%d\t%d\t.\t+\t.\tID=g%d\n" % (c, s + 1, e, i)
                          for i, (c, s, e) in enumerate(zip(a_chrom.tolist(), a_start.tolist(), a_end.tolist()))],
                         a_chrom, a_start, a_end)
    r_start = rng.integers(0, length, n_reg)
    regions = list(zip(names[rng.integers(0, chroms, n_reg)].tolist(), r_start.tolist(),
                       (r_start + rng.integers(1000, 50000, n_reg)).tolist()))
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        kept = pp.featuresNear(recs, regions, w)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    pick = np.sort(rng.choice(n_feat, max(1, n_feat // 100), replace=False))
    t0 = time.perf_counter()
    want = brute_force(a_chrom[pick].tolist(), a_start[pick].tolist(), a_end[pick].tolist(), regions, w)
    bt = time.perf_counter() - t0
    got = pp.window_u(a_chrom[pick], a_start[pick], a_end[pick], [r[0] for r in regions], [r[1] for r in regions],
                      [r[2] for r in regions], w)
    assert got.tolist() == want
    print(json.dumps({"features": n_feat, "regions": n_reg, "w": w, "kept": len(kept), "featuresNear_s": round(best, 3),
                      "features_per_s": round(n_feat / best), "brute_force_sample": int(pick.size),
                      "brute_force_s": round(bt, 3), "brute_force_features_per_s": round(pick.size / bt)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--features", type=int, default=3_000_000)
    ap.add_argument("--regions", type=int, default=10_000)
    a = ap.parse_args()
    if a.time:
        timing(a.features, a.regions)
    else:
        write_golden()


if __name__ == "__main__":
    main()
