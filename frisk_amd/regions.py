"""python -m frisk_amd.regions: score arbitrary regions against the host profile on the device.

The scanner (python -m frisk_amd) scores the windows of one (w, inc) grid.  This module scores the regions a BED or GFF file
names - merged anomalies, refined boundaries, genes - each as the slice it is, with the same k-mer profile, the same IVOM / KLD,
GC and RIP arithmetic (Engine.score_ranges -> frisk_score_ranges, csrc/range_kernels.h):

    python -m frisk_amd.regions -H host.fa --gff genes.gff3 --gffFeatures gene          which genes are themselves foreign?
    python -m frisk_amd.regions -H donor.fa -Q query.fa --bed anomalies.bed             where did these regions come from?

-H, -Q, -m, -k, -t, --maskHost, --recalc and --RIP are the main command line's, with the same defaults and the same inverted
--recalc (giving it forces recomputation); the genome k-mer cache file in --tempDir is the main command line's too, read when it
is there and written when it is not.  Exactly one of --bed and --gff names the regions:
    BED   columns 1-3, 0-based half-open; an optional column 4 is the id; `#`, `track` and `browser` lines are skipped
    GFF   read as --gffIn reads it (postprocess.read_gff), 1-based inclusive; the id is the ID= attribute, else `.`
Output (-O, in --tempDir): header `name start stop length windowKLD GC [PI SI CRI] id note`, one row per input record in input
order, start / stop 1-based inclusive, floats as in the score table.  note: `.`, `unresolved` (30 % or more of the region is not
uppercase A/C/G/T: not scored, as the reference drops such a window), `ZeroDivisionError` (where the reference would raise it) or
`noMaxmer` (no valid max-mer: the KLD is the int 0).  A record that names an unknown scaffold or reaches past its end ends the
run with exit status 1 and a message naming the record; it is not clipped.

    python -m frisk_amd.regions -H host.fa -Q query.fa --bed anomalies.bed --donors d1.fa d2.fa     which donor is nearest?

--donors scores every region against the host's profile AND each donor's in one pass over the regions (Engine.score_ranges_panel ->
frisk_score_ranges_panel, csrc/panel_kernels.h: a region is counted once).  Labels are the FASTA basenames, the host's included;
two equal labels end the run with exit status 1.  Each donor's genome k-mer cache is the file the main command line uses with that
FASTA as -H: read when it is there and --recalc was not given, written otherwise; --maskHost applies to every profile.  -O is
byte for byte the file of the same run without --donors.  --donorOutfile (in --tempDir): header `name start stop length id <host
label> <donor labels, command-line order> nearest margin`, one row per input record; a cell is the KLD as -O would print it under
that profile (the int 0 for noMaxmer, nan for unresolved / ZeroDivisionError), `nearest` the label of the smallest non-NaN cell
(the first in column order wins a tie; `.` for none), `margin` the second smallest minus the smallest (`.` with fewer than two).

    python -m frisk_amd.regions -H host.fa --gff genes.gff3 --null markov --nullDraws 200      is this KLD unusual at this length?

The KLD of a slice depends on its length as much as on its content, so windowKLD cannot be read across regions.  --null scores,
for every distinct region length, --nullDraws null sequences of that length against the same profile (HotPath.nullScores) and
places each region in the null distribution of its own length:
    --null markov   sequences drawn on the device from the Markov chain of the host's own k-mer profile (frisk_seq_null,
                    nullmodel.py; order --nullOrder r, default kmax - 1, kmin <= r + 1 <= kmax): what sampling noise alone does at
                    this length under the host's k-mer model
    --null host     slices of the host itself at seeded positions (nullmodel.host_draws): what this genome looks like at this
                    length, heterogeneity included
--seed S (default 0) fixes the draws.  -O is byte for byte the file of the same run without --null.  --nullOutfile (in --tempDir,
default region_null_scores.tsv): header `name start stop length id windowKLD nullN nullMean nullSD excess z p note`, one row per
input record in input order, windowKLD and note as in -O.  nullN = the null draws whose own note is `.`; nullMean, nullSD (n - 1 in
the divisor) their mean and standard deviation; excess = windowKLD - nullMean; z = excess / nullSD; p = (1 + #{null >= windowKLD})
/ (1 + nullN) - ties count against the region.  A field that does not exist is `.`: all six for a record whose note is not `.` or
without a valid draw, nullSD and z with a single draw, z with nullSD 0.
The null is matched on the region's plain length, not on its count of valid bases.  Host draws may overlap the region itself, as
the scanner's percentile includes the window it judges.  --null does not go with --donors.

    python -m frisk_amd.regions -H host.fa --bed anomalies.bed --topKmers 20                   which k-mers drive this KLD?

A region's KLD is a sum over its present max-mers (the words of --maxWordSize letters it holds) of term = pw * log2(pw / pg), pw
and pg the region's and the host's interpolated probabilities of the word.  --topKmers N (1..64, off by default) lists each region's
N largest terms.  The regions are then scored by the one call that also keeps the terms (HotPath.explainRegions ->
frisk_explain_ranges, csrc/explain_kernels.h): -O is byte for byte the file of the same run without --topKmers.  --kmerOutfile (in
--tempDir, default region_kmers.tsv): header `name start stop id rank kmer count pw pg term share`; a region whose note is `.` gets
min(N, its distinct max-mers) lines, regions in input order, rank from 1 (the largest term; equal terms in the tables' digit order
A, T, G, C); a region with any other note gets none.  kmer = the word, count = its occurrences in the region (overlapping, the
region upper-cased), share = term / windowKLD (`.` when the KLD is 0), floats as in -O.  The term of an over-represented word is
positive, that of a present but under-represented word negative - a KLD is what is left after they cancel, so shares can exceed 1
and the tail of a short region's list, which holds every word it has, is negative.  --topKmers goes with --null (the terms are
taken before the null batch replaces the resident one) and not with --donors.

    python -m frisk_amd.regions -H host.fa --bed anomalies.bed --refine 2000                   where does each region start and end?

Every region the scanner yields has boundaries on a window grid.  --refine F moves each boundary, within F bases on either side, to a
likelihood-ratio change point (HotPath.refineRegions -> frisk_refine_ranges, csrc/refine_kernels.h; refine.py is the definition): a
Markov chain of order --refineOrder r is trained on the region's core - the region without min(F, length / 4) bases at each end,
where it is certainly the island - and compared base by base with the host's chain over both flanks; each boundary goes where the
cumulative log-likelihood ratio is extreme, and on a tie the shorter region wins.  The default order is min(max(2, kmin - 1), kmax -
1): LOW on purpose - a core of a few kilobases cannot train a long context, and at order 5 the cut is off by kilobases (DESIGN.md
section 17).  -O is byte for byte the file of the same run without --refine; the refined regions are scored by a second call on the
still-resident query.  --refineOutfile (in --tempDir, default region_refined.tsv): header `name start stop length id newStart newStop
newLength shiftStart shiftStop llrStart llrStop flank windowKLD newKLD note`, one row per input record in input order; coordinates
1-based inclusive as in -O; shift = new minus old; llr = what the move gains in log-likelihood ratio, in bits; flank = the bases
searched on either side of a boundary; windowKLD / newKLD = the region's and the refined region's KLD as -O prints one.  note: `.`,
`unresolved` (30 % or more of the core is not uppercase A/C/G/T: left as it was) or `short` (fewer than 4 bases: left as it was).
--refinedBed (in --tempDir, default regions_refined.bed): name, newStart, newStop (0-based half-open), id - ready to be fed back
through --bed.  --refine does not go with --donors, --null or --topKmers: a second run on the refined BED gives those.
"""
import argparse
import gzip
import logging
import os
import pickle
import sys

from . import _ffi
from . import cli
from . import postprocess as pp


def build_parser():
    p = argparse.ArgumentParser(prog="frisk-regions", description="Score the regions of a BED / GFF file against the host's "
                                "k-mer profile (KLD, GC, RIP indices), each region as a whole.")
    p.add_argument("-H", "--hostSeq", type=str, required=True, help="host genome FASTA (one species)")
    p.add_argument("-Q", "--querySeq", type=str, default=None, help="the regions lie in this FASTA (default: the host)")
    p.add_argument("-O", "--outfile", type=str, default="region_scores.tsv", help="score table of the regions, written in --tempDir")
    p.add_argument("-t", "--tempDir", type=str, default="temp", help="working / output directory")
    p.add_argument("-m", "--minWordSize", type=int, default="1", help="shortest k-mer")
    p.add_argument("-k", "--maxWordSize", type=int, default="8", help="longest k-mer")
    p.add_argument("--maskHost", action="store_true", default=False, help="skip soft-masked k-mers when profiling the host")
    p.add_argument("--recalc", action="store_false", default=True, help="force recomputation of the host k-mer profile")
    p.add_argument("--RIP", action="store_true", default=False, help="report RIP indices per region")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--bed", type=str, default=None, help="regions as BED: columns 1-3, optional id in column 4")
    src.add_argument("--gff", type=str, default=None, help="regions as GFF records")
    p.add_argument("--gffFeatures", type=str, nargs="+", default=None, help="with --gff: keep records of these types (column 3)")
    p.add_argument("--donors", type=str, nargs="+", default=None, help="candidate donor genomes (FASTA): score every region against "
                   "each of them too, in the same pass, and name the nearest profile")
    p.add_argument("--donorOutfile", type=str, default="region_donor_scores.tsv", help="with --donors: the per-donor KLD table, "
                   "written in --tempDir")
    p.add_argument("--null", type=str, choices=["markov", "host"], default=None, help="place every region in a null distribution of "
                   "its own length: sequences drawn from the host profile's Markov chain, or slices of the host")
    p.add_argument("--nullDraws", type=int, default=100, help="with --null: null sequences per distinct region length")
    p.add_argument("--nullOrder", type=int, default=None, help="with --null markov: order r of the chain (default: kmax - 1)")
    p.add_argument("--seed", type=int, default=0, help="with --null: seed of the draws")
    p.add_argument("--nullOutfile", type=str, default="region_null_scores.tsv", help="with --null: the calibrated table, written in "
                   "--tempDir")
    p.add_argument("--topKmers", type=int, default=None, help="list the N (1..64) k-mers of --maxWordSize letters with the largest "
                   "terms of each region's KLD")
    p.add_argument("--kmerOutfile", type=str, default="region_kmers.tsv", help="with --topKmers: the per-region k-mer table, written "
                   "in --tempDir")
    p.add_argument("--refine", type=int, default=None, metavar="F", help="move each region's boundaries, within F bases (1..65536) on "
                   "either side, to a likelihood-ratio change point")
    p.add_argument("--refineOrder", type=int, default=None, help="with --refine: order r of the two Markov chains (default: "
                   "min(max(2, kmin - 1), kmax - 1); keep it low)")
    p.add_argument("--refineOutfile", type=str, default="region_refined.tsv", help="with --refine: the table of refined boundaries, "
                   "written in --tempDir")
    p.add_argument("--refinedBed", type=str, default="regions_refined.bed", help="with --refine: the refined regions as BED, written "
                   "in --tempDir")
    return p


def read_bed(path):
    """[(name, start, stop, id)] of a BED file (plain or gzip), 0-based half-open as BED is; id = column 4, else '.'.
    Skipped: blank lines and lines that start with '#', `track` or `browser`.  ValueError names the file and the line otherwise."""
    with open(path, "rb") as fh:
        magic = fh.read(2)
    out = []
    with (gzip.open if magic == b"\x1f\x8b" else open)(path, "rt", encoding="utf-8", errors="surrogateescape", newline="\n") as fh:
        for no, raw in enumerate(fh, 1):
            line = raw.rstrip("\r\n")
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            f = line.split("\t")
            if len(f) < 3:
                raise ValueError("%s, line %d: %d tab-separated fields, a BED record has at least 3" % (path, no, len(f)))
            try:
                a, b = int(f[1]), int(f[2])
            except ValueError:
                raise ValueError("%s, line %d: start %r and end %r must be integers" % (path, no, f[1], f[2])) from None
            if a < 0 or b <= a:
                raise ValueError("%s, line %d: an empty or negative range %d-%d" % (path, no, a, b))
            out.append((f[0], a, b, f[3] if len(f) > 3 and f[3] else "."))
    return out


def gff_id(line):
    """The ID= attribute of a GFF record's text, else '.'."""
    for attr in line.rstrip("\n").split("\t")[8].split(";"):
        attr = attr.strip()
        if attr.startswith("ID="):
            return attr[3:] or "."
    return "."


def read_gff_regions(path, feature_types=None):
    """[(name, start, stop, id)] of a GFF file's records, 0-based half-open: [column 4 - 1, column 5)."""
    rec = pp.read_gff(path, feature_types)
    return [(str(c), int(a), int(b), gff_id(line)) for line, c, a, b in zip(rec.lines, rec.chrom, rec.start, rec.end)]


def columns(rip):
    return ["name", "start", "stop", "length", "windowKLD", "GC"] + (["PI", "SI", "CRI"] if rip else []) + ["id", "note"]


def region_cell(status, kld):
    """(note, KLD as it is printed) of one row under one profile: the int 0 of an empty sum (L465) for `noMaxmer`."""
    st = int(status)
    if not st & _ffi.ROW_KEPT:
        note = "unresolved"
    elif st & _ffi.ROW_ZERO_WEIGHT:
        note = "ZeroDivisionError"
    elif st & _ffi.ROW_NO_MAXMER:
        note = "noMaxmer"
    else:
        note = "."
    return note, (0 if note == "noMaxmer" else float(kld))


def region_rows(regions, res, rip, fmt):
    """One tab-separated line per region, in input order; start / stop 1-based inclusive."""
    for r, (name, a, b, ident) in enumerate(regions):
        note, kld = region_cell(res.status[r], res.kld[r])
        vals = [name, a + 1, b, b - a, kld, float(res.gc[r])]
        if rip:
            vals += [float(res.pi[r]), float(res.si[r]), float(res.cri[r])]
        yield "\t".join([fmt(v) for v in vals] + [ident, note]) + "\n"


def nearest_margin(cells):
    """(index of the smallest non-NaN cell or None, second smallest minus smallest or None) of one region's KLDs, one per
    profile in column order.  The first in column order wins a tie - and ties are real: a region with a single present max-mer
    has KLD 0 against every profile.  No margin with fewer than two non-NaN cells."""
    best = sorted((v, i) for i, v in enumerate(cells) if v == v)
    if not best:
        return None, None
    return best[0][1], (best[1][0] - best[0][0] if len(best) > 1 else None)


def donor_columns(labels):
    return ["name", "start", "stop", "length", "id"] + list(labels) + ["nearest", "margin"]


def donor_rows(regions, panel, planes, labels, fmt):
    """One line per region of the per-donor table: the KLD against each profile (plane planes[i] of `panel` under labels[i]),
    printed as region_rows prints it for that profile, then the nearest profile's label and its margin (`.` for none)."""
    for r, (name, a, b, ident) in enumerate(regions):
        cells = [region_cell(panel.status[p][r], panel.kld[p][r])[1] for p in planes]
        near, margin = nearest_margin(cells)
        yield "\t".join([fmt(v) for v in [name, a + 1, b, b - a]] + [ident] + [fmt(v) for v in cells] +
                        ["." if near is None else labels[near], "." if margin is None else fmt(margin)]) + "\n"


NULL_COLUMNS = ["name", "start", "stop", "length", "id", "windowKLD", "nullN", "nullMean", "nullSD", "excess", "z", "p", "note"]


def null_problem(args, regions):
    """Why this command line cannot have its --null (a message), or None: checked before any device work."""
    if args.donors:
        return "--null does not go with --donors"
    if args.nullDraws < 1:
        return "--nullDraws must be at least 1"
    if args.nullOrder is not None:
        if args.null == "host":
            return "--nullOrder goes with --null markov"
        if not args.minWordSize <= args.nullOrder + 1 <= args.maxWordSize:
            return "--nullOrder r needs the k-mers of length r + 1: %d <= r + 1 <= %d" % (args.minWordSize, args.maxWordSize)
    if args.null == "markov" and regions:
        from . import nullmodel
        longest = max(b - a for _, a, b, _ in regions)
        if not nullmodel.batch_fits(args.nullDraws, longest):
            return "--nullDraws %d sequences of %d bases (the longest region) are more than one batch can hold" % (args.nullDraws, longest)
    return None


def null_rows(regions, res, lengths, kld, valid, fmt):
    """One line per region of the --null table.  `lengths`: the distinct lengths that were drawn; kld, valid: HotPath.nullScores'."""
    from . import nullmodel
    row_of = {n: i for i, n in enumerate(lengths)}
    for r, (name, a, b, ident) in enumerate(regions):
        note, cell = region_cell(res.status[r], res.kld[r])
        fields = [None] * 6
        if note == ".":
            i = row_of[b - a]
            fields = nullmodel.stats(cell, kld[i][valid[i]])
        yield "\t".join([fmt(v) for v in [name, a + 1, b, b - a]] + [ident, fmt(cell)] +
                        ["." if v is None else fmt(v) for v in fields] + [note]) + "\n"


KMER_COLUMNS = ["name", "start", "stop", "id", "rank", "kmer", "count", "pw", "pg", "term", "share"]


def kmers_problem(args):
    """Why this command line cannot have its --topKmers (a message), or None: checked before any device work."""
    if not 1 <= args.topKmers <= _ffi.EXPLAIN_MAX:
        return "--topKmers takes 1..%d" % _ffi.EXPLAIN_MAX
    if args.donors:
        return "--topKmers does not go with --donors"
    return None


def kmer_text(code, k):
    """The k letters of a table code: digits A, T, G, C = 0..3, first base most significant."""
    code = int(code)
    return "".join("ATGC"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_rows(regions, res, k, fmt):
    """The lines of the --topKmers table: for each region whose note is `.`, its filled slots in rank order."""
    for r, (name, a, b, ident) in enumerate(regions):
        note, kld = region_cell(res.status[r], res.kld[r])
        if note != ".":
            continue
        for j in range(min(int(res.n_present[r]), res.code.shape[1])):
            term = float(res.term[r][j])
            share = "." if kld == 0 else fmt(term / kld)
            yield "\t".join([fmt(v) for v in [name, a + 1, b]] + [ident, fmt(j + 1), kmer_text(res.code[r][j], k),
                             fmt(int(res.count[r][j])), fmt(float(res.pw[r][j])), fmt(float(res.pg[r][j])), fmt(term), share]) + "\n"


REFINE_COLUMNS = ["name", "start", "stop", "length", "id", "newStart", "newStop", "newLength", "shiftStart", "shiftStop", "llrStart",
                  "llrStop", "flank", "windowKLD", "newKLD", "note"]


def refine_order(args):
    """The order of --refine's chains: --refineOrder, else low (refine.default_order)."""
    from . import refine
    return refine.default_order(args.minWordSize, args.maxWordSize) if args.refineOrder is None else args.refineOrder


def refine_problem(args):
    """Why this command line cannot have its --refine (a message), or None: checked before any device work."""
    for other, given in (("--donors", args.donors), ("--null", args.null), ("--topKmers", args.topKmers is not None)):
        if given:
            return "--refine does not go with %s: run again on the refined BED for that" % other
    if not 1 <= args.refine <= _ffi.REFINE_MAX_FLANK:
        return "--refine takes 1..%d bases" % _ffi.REFINE_MAX_FLANK
    r = refine_order(args)
    if r < 0 or not args.minWordSize <= r + 1 <= args.maxWordSize:
        return "--refineOrder r needs the k-mers of length r + 1: %d <= r + 1 <= %d" % (args.minWordSize, args.maxWordSize)
    return None


def refine_note(status, flank_used):
    st = int(status)
    return "short" if int(flank_used) == 0 else ("." if st & _ffi.ROW_KEPT else "unresolved")


def refine_rows(regions, res, rf, res_new, fmt):
    """One line per region of the --refine table.  res, res_new: the score columns of the regions and of the refined regions."""
    for r, (name, a, b, ident) in enumerate(regions):
        ns, ne = int(rf.new_start[r]), int(rf.new_stop[r])
        llr = [float(int(g)) / 4294967296.0 for g in (rf.gain_start[r], rf.gain_stop[r])]
        yield "\t".join([fmt(v) for v in [name, a + 1, b, b - a]] + [ident] +
                        [fmt(v) for v in [ns + 1, ne, ne - ns, ns - a, ne - b, llr[0], llr[1], int(rf.flank_used[r]),
                                          region_cell(res.status[r], res.kld[r])[1], region_cell(res_new.status[r], res_new.kld[r])[1]]] +
                        [refine_note(rf.status[r], rf.flank_used[r])]) + "\n"


def refined_bed_rows(regions, rf):
    for r, (name, _, _, ident) in enumerate(regions):
        yield "%s\t%d\t%d\t%s\n" % (name, int(rf.new_start[r]), int(rf.new_stop[r]), ident)


def write_table(path, columns, rows=()):
    """A table of the command line: the header, then the rows' lines."""
    with open(path, "w") as fh:
        fh.write("\t".join(columns) + "\n")
        fh.writelines(rows)


def _load_pickle(path, log):
    log.info("Importing previously calculated genome kmers from %s", path)
    with open(path, "rb") as fh:
        return pickle.load(fh, encoding="latin1")


def _dump_pickle(path, maps):
    tmp = path + ".tmp%d" % os.getpid()
    with open(tmp, "wb") as fh:
        pickle.dump(maps, fh, protocol=2)
    os.replace(tmp, path)


def score_with_donors(args, hp, regions, log):
    """--donors: the host's and every donor's profile into the engine's panel - each from its genome k-mer cache (the file the main
    command line would use with that FASTA as -H) when it is there and --recalc was not given, computed and cached otherwise -,
    then one pass over the regions.  Returns (PanelResult, [plane of the host, planes of the donors])."""
    from .hotpath import profileToMaps
    paths = [args.hostSeq] + list(args.donors)
    caches, have = {}, {}
    for path in paths:
        one = argparse.Namespace(**vars(args))
        one.hostSeq = path
        caches[path] = cli.makePicklePath(one, "genome")
        if os.path.isfile(caches[path]) and args.recalc:
            have[path] = _load_pickle(caches[path], log)
        else:
            log.info("Calculating kmers for %s sequence: %s", "host" if path == args.hostSeq else "donor", path)
    panel, host, donors = hp.scoreRegionsPanel(args, args.querySeq or args.hostSeq, [r[:3] for r in regions], args.donors,
                                               genomeKmers=have.get(args.hostSeq),
                                               donorKmers={p: have[p] for p in args.donors if p in have})
    for path, arrays in hp.panelProfiles.items():
        _dump_pickle(caches[path], profileToMaps(*arrays, args.minWordSize, args.maxWordSize))
    return panel, [host] + list(donors)


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    log = logging.getLogger("frisk_amd")
    if args.minWordSize > args.maxWordSize:
        logging.error("[ERROR] Minimum kmer size (-m/--minWordSize) must be less than Maximum kmer size (-k/--maxWordSize)\n")
        return 1
    if args.gffFeatures and not args.gff:
        logging.error("[ERROR] --gffFeatures goes with --gff\n")
        return 1
    problem = kmers_problem(args) if args.topKmers is not None else None
    if problem:
        logging.error("[ERROR] %s\n", problem)
        return 1
    problem = refine_problem(args) if args.refine is not None else None
    if problem:
        logging.error("[ERROR] %s\n", problem)
        return 1
    labels = [os.path.basename(p) for p in [args.hostSeq] + list(args.donors or [])]
    if len(set(labels)) != len(labels):
        logging.error("[ERROR] the host and the donors (--donors) must differ in their file names, which label the columns: %s\n",
                      " ".join(labels))
        return 1
    try:
        regions = read_bed(args.bed) if args.bed else read_gff_regions(args.gff, args.gffFeatures)
    except (OSError, ValueError) as err:
        logging.error("[ERROR] %s\n", err)
        return 1
    problem = null_problem(args, regions) if args.null else None
    if problem:
        logging.error("[ERROR] %s\n", problem)
        return 1
    rip = bool(args.RIP) and args.minWordSize <= 2
    if not os.path.isdir(os.path.abspath(args.tempDir)):
        os.makedirs(os.path.abspath(args.tempDir))
    out_path, kmer_path, null_path, donor_path = (os.path.join(args.tempDir, f) for f in (args.outfile, args.kmerOutfile, args.nullOutfile,
                                                                                         args.donorOutfile))
    refine_path, bed_path = os.path.join(args.tempDir, args.refineOutfile), os.path.join(args.tempDir, args.refinedBed)
    if not regions:
        write_table(out_path, columns(rip))
        if args.donors:
            write_table(donor_path, donor_columns(labels))
        if args.null:
            write_table(null_path, NULL_COLUMNS)
        if args.topKmers is not None:
            write_table(kmer_path, KMER_COLUMNS)
        if args.refine is not None:
            write_table(refine_path, REFINE_COLUMNS)
            open(bed_path, "w").close()
        log.info("No regions in %s: wrote the header to %s", args.bed or args.gff, out_path)
        return 0

    from .hotpath import HotPath
    genomepickle = cli.makePicklePath(args, "genome")
    hp = HotPath(args.minWordSize, args.maxWordSize, device=0, cache_dir=args.tempDir, use_cache=bool(args.recalc))
    panel = None
    try:
        genomeKmers = None
        if args.donors:
            pass                                                # (every profile's cache is score_with_donors' business)
        elif os.path.isfile(genomepickle) and args.recalc:      # --recalc is store_false: giving it forces recomputation
            genomeKmers = _load_pickle(genomepickle, log)
        else:
            log.info("Calculating kmers for host sequence: %s", args.hostSeq)
        try:
            if args.donors:
                panel, planes = score_with_donors(args, hp, regions, log)
                res = panel.plane(planes[0])
            elif args.refine is not None:       # the boundaries first; both scorings on the query it leaves resident
                rf = hp.refineRegions(args, args.querySeq or args.hostSeq, [r[:3] for r in regions], args.refine, refine_order(args),
                                      genomeKmers=genomeKmers)
                res = hp.scoreResident(args, rf.seq_index, rf.start, rf.stop)
                res_new = hp.scoreResident(args, rf.seq_index, rf.new_start, rf.new_stop)
            elif args.topKmers is not None:
                res = hp.explainRegions(args, args.querySeq or args.hostSeq, [r[:3] for r in regions], args.topKmers,
                                        genomeKmers=genomeKmers)
            else:
                res = hp.scoreRegions(args, args.querySeq or args.hostSeq, [r[:3] for r in regions], genomeKmers=genomeKmers)
        except ValueError as err:
            logging.error("[ERROR] %s\n", err)
            return 1
        if genomeKmers is None and not args.donors:
            _dump_pickle(genomepickle, hp.profileMaps())
        if args.null:       # (after the regions: the markov null replaces the resident batch)
            lengths = sorted({b - a for r, (_, a, b, _) in enumerate(regions) if region_cell(res.status[r], res.kld[r])[0] == "."})
            null_kld, null_valid = hp.nullScores(args, lengths, args.nullDraws, args.seed, args.null, order=args.nullOrder)
    finally:
        hp.close()
    write_table(out_path, columns(rip), region_rows(regions, res, rip, cli._fmt()))
    log.info("Scored %d regions: %s", len(regions), out_path)
    if args.refine is not None:
        write_table(refine_path, REFINE_COLUMNS, refine_rows(regions, res, rf, res_new, cli._fmt()))
        with open(bed_path, "w") as fh:
            fh.writelines(refined_bed_rows(regions, rf))
        log.info("Refined their boundaries within %d bases (order %d): %s, %s", args.refine, refine_order(args), refine_path, bed_path)
    if args.topKmers is not None:
        write_table(kmer_path, KMER_COLUMNS, kmer_rows(regions, res, args.maxWordSize, cli._fmt()))
        log.info("Listed the %d largest KLD terms of each: %s", args.topKmers, kmer_path)
    if args.null:
        write_table(null_path, NULL_COLUMNS, null_rows(regions, res, lengths, null_kld, null_valid, cli._fmt()))
        log.info("Placed them in %s nulls of %d draws per length (%d lengths): %s", args.null, args.nullDraws, len(lengths), null_path)
    if panel is not None:
        write_table(donor_path, donor_columns(labels), donor_rows(regions, panel, planes, labels, cli._fmt()))
        log.info("Scored them against %d donor genomes: %s", len(args.donors), donor_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
