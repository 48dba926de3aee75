"""What the --gffIn tests share: the brute-force statement of `bedtools window -w W -u` (one Python step per pair of records, no
sorting, no numpy), readers of the GFF files a run writes, and the seeded random cases."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTA = os.path.join(GOLD, "inputs", "markov_islands.fa")
GFF = os.path.join(GOLD, "inputs", "markov_islands.gff3")      # hand-written for FASTA


def brute_mask(a, b, w):
    """a, b: records (chrom, start, end) in half-open BED numbers.  True for every a that shares a base with some b of its chrom
    after being widened by w (start clipped at 0)."""
    mask = []
    for ac, a0, a1 in a:
        lo, hi = max(0, a0 - w), a1 + w
        hit = False
        for bc, b0, b1 in b:
            if bc == ac and lo < b1 and b0 < hi:
                hit = True
        mask.append(hit)
    return mask


def gff_rows(path):
    """(line, fields) of every data line of a GFF file written by a run or committed as a fixture."""
    out = []
    with open(path, newline="") as fh:
        for line in fh:
            if line.strip() and not line.startswith("#"):
                out.append((line, line.rstrip("\n").split("\t")))
    return out


def gff_as_bed(rows, types=None):
    """GFF data lines as BED records (chrom, start - 1, end), optionally of the given types only."""
    return [(f[0], int(f[3]) - 1, int(f[4])) for _line, f in rows if types is None or f[2] in types]


def expected_lines(types, regions, w, path=GFF):
    """The lines of the annotation a run must keep: its records of the given types, brute force against `regions`."""
    rows = [(line, f) for line, f in gff_rows(path) if f[2] in types]
    mask = brute_mask(gff_as_bed(rows), regions, w)
    return [line for (line, _f), m in zip(rows, mask) if m]


RANDOM_CASES = 200
RANDOM_W = (0, 1, 7, 1000)


def random_case(no):
    """Case `no` of the seeded set: 0-60 features, 0-20 regions, 1-3 chrom names (the regions may also sit on one the features
    never use), w from RANDOM_W in turn.  Starts lie on a grid of 5 moved by -1 / 0 / +1 and lengths are short, so that book-ended
    pairs, one-base overlaps and gaps of exactly w are common."""
    rng = np.random.default_rng(1000 + no)
    names = ["c1", "c2", "c10"][:int(rng.integers(1, 4))]

    def draw(n, pool):
        start = np.maximum(rng.integers(0, 24, n) * 5 + rng.choice([-1, 0, 0, 1], n), 0)
        end = start + rng.choice([1, 1, 2, 4, 5, 6, 10, 30], n)
        return [(pool[int(c)], int(s), int(e)) for c, s, e in zip(rng.integers(0, len(pool), n), start, end)]
    a = draw(int(rng.integers(0, 61)), names)
    b = draw(int(rng.integers(0, 21)), names + ["cX"])
    return a, b, RANDOM_W[no % len(RANDOM_W)]
