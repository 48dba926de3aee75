"""`frisk` command line on the GPU hot path (SURVEY.md section 8, rows a11/a12 + f2 + f1).

Same option surface as the reference's argparse block (frisk/__init__.py L1127-1398: names, types, defaults,
choices, the inverted store_false semantics of --recalc/--recalcWin), same files in --tempDir (score table,
caches, GFF3) and the same row echo on stdout.  Phase A and phase B run through libfrisk_hip.so
(frisk_amd.hotpath); thresholds, merging and GFF3 writing are host numpy (frisk_amd.postprocess).

--hmmKLD runs frisk_amd.hmm (own 2-state Gaussian HMM; hmmlearn is absent and seeds randomly - parity unpinned).
--runProjection PCA, PY-TSNE (the reference's exact t-SNE, Y0 seeded by --seed, 0 when not given), MDS (sklearn's metric MDS,
its starts seeded the same way) or IncrementalPCA (sklearn's, in batches of 5 F rows) with --cluster DBSCAN / KMEANS runs
frisk_amd.projection on the GPU and writes the cluster-labelled GFF3.
--runProjection NMF (sklearn's coordinate-descent NMF from the nndsvda start, seeded the same way) runs on the GPU too and, with
--dumpPCAdata, writes the projection as the pickle anomNMF; --cluster after NMF is still reported as unavailable (no cluster GFF3).
--updateHMM (with --updateWin / --updateInc; the reference advertises them as a future function and never wired them) scans the
query again with the fine window, segments that track with the device HMM (csrc/hmm_kernels.h), writes it to
updateWin_<w>_inc_<i>_<hmmOutfile>, and - with --gffOutfile - writes the anomalies with every boundary moved to the nearest
boundary of the fine track (the reference's unused updateHMM, L737-755) to HMMupdated_<gffOutfile>.  No other output changes.
Skipped with a warning in a sharded job, under --exitAfter, and where the fine scan meets the reference's ZeroDivisionError.
--gffIn with --gffFeatures (and --gffRange, 0 when not given) is the reference's last step before plotting (L1709-1747): the
records of the annotation whose type is one of --gffFeatures and that lie within --gffRange bases of an anomaly go to
featuresIn_thresholded_Anomalies_<basename of gffIn>, and with --hmmKLD those near a State1 / State2 interval of the main track to
featuresIn_hmm_State1_<basename> / featuresIn_hmm_State2_<basename> - `bedtools window -w gffRange -u` restated on the host
(frisk_amd.postprocess.window_u); a file is written only when it has a record.  Rank 0, not under --exitAfter; no other output changes.
--cluster SPECTRAL (sklearn's SpectralClustering: rbf affinities, normalised Laplacian, k-means on the top --kClusters
eigenvectors, seeded the same way) runs on the GPU after PCA, PY-TSNE, MDS or IncrementalPCA and, with --dumpPCAdata, writes its
labels as the pickle anomSPECTRAL; it is still reported as unavailable and writes no cluster GFF3 (CLUSTERINGS_UNWRITTEN).
--runProjection SKL-TSNE (sklearn 1.7's TSNE with the reference's parameters, --tsneGradient barnes_hut | exact and --tsneInitPCA
random | pca, seeded the same way) runs on the GPU and logs its iterations, KL divergence and timings; with --dumpPCAdata it writes
the embedding as the pickle anomSKLTSNE.  barnes_hut keeps sklearn's nearest-neighbour affinities but sums the repulsive term over
all pairs: sklearn's angle -> 0 limit, not its angle = 0.5 tree approximation; pca starts from the exact PCA, not sklearn's
randomized one.  --cluster after SKL-TSNE is still reported as unavailable and writes no cluster GFF3
(PROJECTIONS_DUMPED).
--spikeNormal (with --runProjection; the reference advertises it as a future function and never wired it) puts ordinary windows
into the projection beside the anomalies: as many as there are anomalous rows, the unpicked windows whose log10(KLD) lies nearest
the median of all scored windows (frisk_amd.postprocess.spike_rows; no random numbers).  The query is loaded by the native reader
and the k-mer vectors of anomalies and spiked windows come from the device kernel on the packed batch (csrc/kvec_kernels.h,
frisk_window_vectors).  The anomaly rows come first, unchanged; the spiked rows follow, labelled name:start:stop.  Projection and
clustering run on all rows; --dumpPCAdata writes all of them and the bool pickle anomSpike; the cluster GFF3 keeps the anomaly
rows (with the classes of the joint clustering) and the spiked rows go to spikeNormal_<cluster GFF3>.  No other output changes.
Out of scope here: --graphics (seaborn/matplotlib).
That option is accepted, as in the reference, and reported as unavailable if used.

Run under `python -m torch.distributed.run --nproc-per-node N -m frisk_amd ...` to shard one job over N GPUs
(frisk_amd.distributed): rank 0 writes the outputs.
"""
import argparse
import logging
import os
import pickle
import sys

import numpy as np

from . import postprocess as pp

log = logging.getLogger("frisk")


def build_parser():
    p = argparse.ArgumentParser(prog="frisk", description="Calculate all kmers in a given sequence")
    p.add_argument("--version", action="version", version="frisk --" + pp.FRISK_VERSION)
    # inputs
    p.add_argument("-H", "--hostSeq", type=str, required=True, help="host genome FASTA (one species)")
    p.add_argument("-Q", "--querySeq", type=str, default=None, help="scan this FASTA against the host profile (default: the host)")
    p.add_argument("--gffIn", type=str, default=None, help="GFF annotation of the scanned genome")
    # outputs
    p.add_argument("-O", "--outfile", type=str, default="raw_window_scores.bed", help="per-window score table, written in --tempDir")
    p.add_argument("-t", "--tempDir", type=str, default="temp", help="working / output directory")
    p.add_argument("--gffOutfile", type=str, default=None, help="GFF3 of merged anomalous features")
    p.add_argument("--hmmOutfile", type=str, default="2StateHmm.gff3", help="GFF3 of HMM state features")
    p.add_argument("--graphics", type=str, default=None, help="PDF of summary graphics")
    # output options
    p.add_argument("--mergeDist", type=int, default=0, help="merge anomalies within this many bases")
    p.add_argument("--gffFeatures", type=str, default=None, nargs="+", help="feature types of --gffIn to intersect with anomalies")
    p.add_argument("--gffRange", type=int, default=0, help="report annotations within this distance of anomalies")
    # core settings
    p.add_argument("-m", "--minWordSize", type=int, default="1", help="shortest k-mer")
    p.add_argument("-k", "--maxWordSize", type=int, default="8", help="longest k-mer")
    p.add_argument("-w", "--windowlen", type=int, default="5000", help="window length")
    p.add_argument("-i", "--increment", type=int, default="2500", help="window step")
    # run settings
    p.add_argument("--maskHost", action="store_true", default=False, help="skip soft-masked k-mers when profiling the host")
    p.add_argument("--exitAfter", default=None, choices=[None, "GenomeKmers", "WindowKLD"], help="stop after this stage")
    p.add_argument("--recalc", action="store_false", default=True, help="force recomputation of the host k-mer profile")
    p.add_argument("--recalcWin", action="store_false", default=True, help="force recomputation of the window scores")
    p.add_argument("--scaffoldsAll", action="store_true", default=False, help="score scaffolds below the minimum size as one window")
    # KLD thresholds
    p.add_argument("--threshTypeKLD", default=None, choices=[None, "percentile", "otsu"], help="how to pick the log10(KLD) cut")
    p.add_argument("--percentileKLD", type=float, default=99.0, help="percentile for --threshTypeKLD percentile")
    p.add_argument("--hmmKLD", action="store_true", default=False, help="2-state HMM segmentation of the KLD track")
    p.add_argument("-F", "--forceThresholdKLD", type=float, default=None, help="raw KLD above which a window is anomalous")
    # RIP
    p.add_argument("--RIP", action="store_true", default=False, help="report RIP indices per window and RIP features")
    p.add_argument("--RIPgff", type=str, default="RIP_annotation.gff3", help="GFF3 of RIP features")
    p.add_argument("--minCRI", type=float, default=0.0)
    p.add_argument("--peakCRI", type=float, default=1.0)
    p.add_argument("--minPI", type=float, default=1.0)
    p.add_argument("--maxSI", type=float, default=1.0)
    # projection / clustering (every projection, DBSCAN and KMEANS built; SPECTRAL runs but writes no GFF3)
    p.add_argument("--runProjection", default=None, choices=[None, "PCA", "PY-TSNE", "SKL-TSNE", "IncrementalPCA", "NMF", "MDS"])
    p.add_argument("--projectionDims", type=int, default=2)
    p.add_argument("--dimReduce", default="windows", choices=["features", "windows"])
    p.add_argument("--cluster", default=None, choices=[None, "DBSCAN", "KMEANS", "SPECTRAL"])
    p.add_argument("--dumpPCAdata", action="store_true", default=False)
    p.add_argument("--spikeNormal", action="store_true", default=False)
    p.add_argument("--pcaMin", type=int, default="1")
    p.add_argument("--pcaMax", type=int, default="6")
    p.add_argument("--perplexity", type=float, default=20.0)
    p.add_argument("--tsneGradient", default="barnes_hut", choices=["barnes_hut", "exact"])
    p.add_argument("--tsneInitPCA", default="random", choices=["random", "pca"])
    p.add_argument("--epsDBSCAN", type=float, default=10)
    p.add_argument("--kClusters", type=int, default=2)
    p.add_argument("--seed", default=None)
    p.add_argument("--chrmlist", default=None, nargs="+")
    p.add_argument("--updateHMM", action="store_true", default=False,
                   help="refine anomaly boundaries to the nearest boundary of a fine-scale HMM track (second scan)")
    p.add_argument("--updateWin", type=int, default=1000, help="window length of the fine scan")
    p.add_argument("--updateInc", type=int, default=500, help="increment of the fine scan")
    p.add_argument("--findSelf", action="store_true", default=False, help="report windows BELOW the threshold instead")
    return p


PROJECTIONS = ("PCA", "PY-TSNE", "MDS", "IncrementalPCA")     # --runProjection methods built here (frisk_amd.projection)
PROJECTIONS_UNCLUSTERED = ("NMF",)      # built here too, but --cluster on them is still reported as unavailable (see unavailable)
PROJECTIONS_DUMPED = ("SKL-TSNE",)      # built here too and treated like PROJECTIONS_UNCLUSTERED: logged, dumped with --dumpPCAdata, unclustered
CLUSTERINGS = ("DBSCAN", "KMEANS")      # --cluster methods built here
CLUSTERINGS_UNWRITTEN = ("SPECTRAL",)   # built here too, but still reported as unavailable and without a cluster GFF3 (see unavailable)


def unavailable(args):
    """(option, reason) of every given option this build accepts but does not run.  --cluster runs only as DBSCAN or KMEANS
    after --runProjection PCA, PY-TSNE, MDS or IncrementalPCA (the reference clusters the projection, L1635-1655).  The NMF
    projection runs (PROJECTIONS_UNCLUSTERED), but clustering it is still reported as unavailable and writes no cluster GFF3:
    tests/test_projection_cluster_cpu.py pins ("NMF", "DBSCAN") to this warning.  Moving "NMF" into PROJECTIONS lifts that.
    --cluster SPECTRAL runs too after one of PROJECTIONS (CLUSTERINGS_UNWRITTEN: its labels are logged and dumped, not written as
    a GFF3), and the same tests pin it to this warning; moving "SPECTRAL" into CLUSTERINGS lifts the fence.  The SKL-TSNE projection
    runs as well (PROJECTIONS_DUMPED) and, like NMF, leaves --cluster reported here."""
    clustering = args.runProjection in PROJECTIONS and args.cluster in CLUSTERINGS
    out = []
    for opt, why in (("cluster", "sklearn clustering is out of scope"), ("graphics", "plotting is out of scope")):
        if getattr(args, opt) and not (opt == "cluster" and clustering):
            out.append((opt, why))
    return out


def mainArgs(argv=None):
    args = build_parser().parse_args(argv)
    if args.minWordSize > args.maxWordSize:
        logging.error("[ERROR] Minimum kmer size (-m/--minWordSize) must be less than Maximum kmer size (-k/--maxWordSize)\n")
        sys.exit(1)
    if args.gffRange < 0:
        logging.error("[ERROR] --gffRange must not be negative, got %s\n", args.gffRange)
        sys.exit(1)
    if args.gffIn and not os.path.isfile(args.gffIn):
        logging.error("[ERROR] --gffIn %s: no such file\n", args.gffIn)
        sys.exit(1)
    return args


def makePicklePath(args, space):
    """Cache file names of the reference (L497-506)."""
    base = os.path.basename(args.hostSeq)
    if space == "genome":
        return os.path.join(args.tempDir, "%s_kmers_%s_%s_genome.p" % (base, args.minWordSize, args.maxWordSize))
    if args.querySeq:
        base = os.path.basename(args.querySeq)
    return os.path.join(args.tempDir, "%s_kmers_%s_%s_KLD_window_%s_increment_%s.p"
                        % (base, args.minWordSize, args.maxWordSize, args.windowlen, args.increment))


def _columns(args):
    if args.RIP and args.minWordSize <= 2:
        return ["name", "start", "stop", "windowKLD", "GC", "PI", "SI", "CRI"]
    return ["name", "start", "stop", "windowKLD", "GC"]


def _fmt():
    return pp.py3_str if os.environ.get("FRISK_FLOAT_REPR", "py2") == "py3" else pp.py2_str


def write_table(path, table, echo=True):
    """Score table exactly as L1475-1494 lays it out: header, one tab-separated row per window, each row also
    printed.  Floats as Python 2's str() prints them (12 significant digits) unless FRISK_FLOAT_REPR=py3.
    The text comes from the library's native formatter in one piece (ScoreTable.text): no per-row Python."""
    fmt = None if _fmt() is pp.py2_str else _fmt()
    raw = getattr(sys.stdout, "buffer", None) if echo else None
    if fmt is None and (raw is not None or not echo):
        # the formatter's bytes go to the file and to stdout as they are (no decode / encode of a few hundred megabytes)
        body = table.text_bytes()
        with open(path, "wb") as fh:
            fh.write(("\t".join(table.columns) + "\n").encode("utf-8"))
            fh.write(body)
        if echo:
            sys.stdout.flush()
            raw.write(body)
            raw.flush()
        return
    body = table.text(fmt)
    with open(path, "w") as fh:
        fh.write("\t".join(table.columns) + "\n")
        fh.write(body)
    if echo:
        sys.stdout.write(body)


def _load_window_cache(path, rip):
    """The window cache the reference pickles is the allWindows DataFrame (L1501); older builds of this package wrote
    {columns, rows}.  Both are read."""
    from .table import ScoreTable
    with open(path, "rb") as fh:
        cached = pickle.load(fh)
    if hasattr(cached, "columns") and hasattr(cached, "itertuples"):
        return ScoreTable.from_frame(cached, rip)
    return ScoreTable.from_rows([tuple(r) for r in cached["rows"]], rip=rip)


def _dump_window_cache(path, table):
    """As the reference: pickle.dump(allWindows DataFrame) (L1501) - so that any tool that reads *_KLD_window_*.p with a current
    pandas can load it.  (Protocol 2 was used here until round 3: under Python 3 it sends
    every numeric column through a latin-1 text detour - 0.5 s per 3 M rows against 0.15 - and no Python 2 pandas reads a frame
    pickled by today's pandas anyway.)  Without pandas: the {columns, rows} form."""
    try:
        obj = table.to_frame()
    except ImportError:
        obj = {"columns": table.columns, "rows": table.rows()}
    with open(path, "wb") as fh:
        # (protocol 5 hands the numeric columns over as buffers instead of copying them into the stream: 0.16 s against 0.24 per
        #  3 M rows, held under the interpreter lock either way; any Python >= 3.8 reads it)
        pickle.dump(obj, fh, protocol=pickle.HIGHEST_PROTOCOL)


def main(argv=None):
    """Entry point.  A process group that this function creates is torn down before it returns."""
    import torch.distributed as dist
    had_group = dist.is_available() and dist.is_initialized()
    try:
        return _main(argv)
    finally:
        if not had_group and dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()


class _Clock:
    """Wall-clock split of one run (logged at the end; FRISK_TIMING=1 also prints it as one JSON line on stderr)."""

    def __init__(self):
        import time
        self._now = time.perf_counter
        self.t0 = self._now()
        self.last = self.t0
        self.parts = []

    def lap(self, label):
        now = self._now()
        self.parts.append((label, now - self.last))
        self.last = now

    def report(self):
        total = self._now() - self.t0
        log.info("timing: " + ", ".join("%s %.3f s" % p for p in self.parts) + ", total %.3f s" % total)
        if os.environ.get("FRISK_TIMING") == "1":
            import json
            sys.stderr.write(json.dumps({"frisk_timing": dict(self.parts), "total_s": total}) + "\n")


FINE_HMM_NATIVE = "gpu"         # GaussianHMM2(native=...) of the fine track: the device model


def _fine_model(device):
    from .hmm import GaussianHMM2
    return GaussianHMM2(native=FINE_HMM_NATIVE, device=device)


def fineTrackName(args):
    return "updateWin_%s_inc_%s_%s" % (args.updateWin, args.updateInc, args.hmmOutfile)


def _fine_scan(args, hp, querySeq, clock):
    """--updateHMM, step 1: the query again with w = --updateWin, inc = --updateInc, same profile, same --scaffoldsAll (no RIP
    columns: nothing reads them).  The table is neither echoed, written nor cached.  None where the reference's scan would die."""
    fine = argparse.Namespace(**vars(args))
    fine.windowlen, fine.increment, fine.RIP = args.updateWin, args.updateInc, False
    try:
        table, _res = hp.scanTable(fine, querySeq)
    except ZeroDivisionError:
        log.warning("--updateHMM skipped: the fine scan (-w %s -i %s) meets a window whose max-mer prefix has zero weight in the "
                    "host profile (the reference's ZeroDivisionError).", args.updateWin, args.updateInc)
        table = None
    clock.lap("fine scan (--updateHMM)")
    return table


def _seed(args):
    # the reference passes random_state=None and leaves numpy unseeded (not reproducible); --seed, 0 when not given, seeds here
    return int(args.seed) if args.seed is not None else 0


def _project(args, anomCounts, device, clock):
    """--runProjection PCA (L1612-1613), PY-TSNE (L1622-1623), MDS (L1624-1627), IncrementalPCA (L1629-1631), NMF (L1632-1636) or
    SKL-TSNE (L1606-1621: sklearn's TSNE; its barnes_hut gradient is the all-pairs angle -> 0 limit, not the angle = 0.5 tree) on
    the anomalies' k-mer proportions, then --cluster DBSCAN / KMEANS on the projection (L1635-1655), except after NMF and SKL-TSNE; --cluster SPECTRAL
    runs there too but returns nothing (_spectral).  Returns the cluster labels (None without a clustering whose GFF3 is written)."""
    from . import projection as P
    if args.runProjection == "PY-TSNE":
        n = anomCounts.shape[0]
        if not 2 <= n <= P.TSNE_MAX_N:
            raise ValueError("PY-TSNE needs between 2 and %d anomalous windows, got %d" % (P.TSNE_MAX_N, n))
        res = P.tsne(anomCounts, args.projectionDims, args.perplexity, seed=_seed(args), device=device,
                     log=lambda it, c: log.info("Iteration %s : error is %s", it, c))
        log.info("PY-TSNE of %s x %s k-mer proportions: mean sigma %s; PCA %.1f ms, affinities %.1f ms, 1000 iterations %.1f ms",
                 n, anomCounts.shape[1], float(np.mean(np.sqrt(1.0 / res.beta))), res.timings["pca_ms"],
                 res.timings["affinities_ms"], res.timings["iterations_ms"])
    elif args.runProjection == "MDS":
        n = anomCounts.shape[0]
        if not 2 <= n <= P.MDS_MAX_N:
            raise ValueError("MDS needs between 2 and %d anomalous windows, got %d" % (P.MDS_MAX_N, n))
        res = P.mds(anomCounts, args.projectionDims, seed=_seed(args), device=device)
        log.info("MDS of %s x %s k-mer proportions: stress %s (start %s of %s, %s iterations); dissimilarities %.1f ms, "
                 "SMACOF %.1f ms", n, anomCounts.shape[1], res.stress, res.best_start + 1, len(res.stresses), res.n_iter,
                 res.timings["dissimilarities_ms"], res.timings["smacof_ms"])
    elif args.runProjection == "IncrementalPCA":
        res = P.incremental_pca(anomCounts, args.projectionDims, device=device)
        log.info("IncrementalPCA of %s x %s k-mer proportions in %s batches: explained variance %s; statistics + Gram %.1f ms, "
                 "eigh %.1f ms, transform %.1f ms", anomCounts.shape[0], anomCounts.shape[1], len(res.batch_sizes),
                 res.explained_variance_.tolist(), res.timings["stats_gram_ms"], res.timings["eigh_ms"],
                 res.timings["transform_ms"])
    elif args.runProjection == "NMF":
        res = P.nmf(anomCounts, args.projectionDims, seed=_seed(args), device=device)
        log.info("NMF of %s x %s k-mer proportions: %s iterations (transform %s), last violation ratio %s; init %.1f ms, "
                 "fit %.1f ms, transform %.1f ms", anomCounts.shape[0], anomCounts.shape[1], res.n_iter, res.transform_n_iter,
                 res.violation_ratios[-1] if res.violation_ratios else 0.0, res.timings["init_ms"], res.timings["fit_ms"],
                 res.timings["transform_ms"])
        if args.dumpPCAdata:                                                # the projection itself, beside anomLabels / anomCounts
            with open(os.path.join(args.tempDir, "anomNMF"), "wb") as fh:
                pickle.dump(res.Y, fh, protocol=2)
    elif args.runProjection == "SKL-TSNE":
        # a perplexity, --projectionDims or number of windows that skl_tsne refuses is a warning: the run goes on as it did before
        # this projection was built
        try:
            res = P.skl_tsne(anomCounts, args.projectionDims, args.perplexity, seed=_seed(args), method=args.tsneGradient,
                             init=args.tsneInitPCA, device=device)
        except ValueError as err:
            log.warning("--runProjection SKL-TSNE skipped: %s", err)
            return None
        log.info("SKL-TSNE (%s, init %s) of %s x %s k-mer proportions: %s iterations, KL divergence %s; affinities %.1f ms, "
                 "start %.1f ms, iterations %.1f ms", args.tsneGradient, args.tsneInitPCA, anomCounts.shape[0], anomCounts.shape[1],
                 res.n_iter + 1, res.kl_divergence, res.timings["affinities_ms"], res.timings["init_ms"],
                 res.timings["iterations_ms"])
        if args.dumpPCAdata:                                                # the embedding itself, beside anomLabels / anomCounts
            with open(os.path.join(args.tempDir, "anomSKLTSNE"), "wb") as fh:
                pickle.dump(res.Y, fh, protocol=2)
    else:
        res = P.pca(anomCounts, args.projectionDims, device=device)
        log.info("PCA of %s x %s k-mer proportions: explained variance %s; covariance %.1f ms, eigh %.1f ms, transform %.1f ms",
                 anomCounts.shape[0], anomCounts.shape[1], res.explained_variance.tolist(), res.timings["cov_ms"],
                 res.timings["eigh_ms"], res.timings["transform_ms"])
    clock.lap(args.runProjection)
    y_pred = None
    if args.runProjection in PROJECTIONS_UNCLUSTERED + PROJECTIONS_DUMPED:
        return None
    if args.cluster == "DBSCAN":
        y_pred = P.dbscan(res.Y, args.epsDBSCAN, device=device)
    elif args.cluster == "KMEANS":
        y_pred = P.kmeans(res.Y, args.kClusters, seed=_seed(args), device=device).labels
    elif args.cluster in CLUSTERINGS_UNWRITTEN:
        _spectral(args, res.Y, device, clock)
    if y_pred is not None:
        log.info("%s: %s clusters, %s unclassified", args.cluster, len(set(y_pred.tolist()) - {-1}), int(np.sum(y_pred == -1)))
        clock.lap(args.cluster)
    return y_pred


def _spectral(args, Y, device, clock):
    """--cluster SPECTRAL (L1659-1662) on the projection Y: the labels are logged and, with --dumpPCAdata, pickled as anomSPECTRAL
    beside anomLabels / anomCounts; no cluster GFF3 follows (CLUSTERINGS_UNWRITTEN).  A --kClusters or a number of windows that
    spectral() refuses is a warning: the run goes on as it did before this clustering was built."""
    from . import projection as P
    try:
        sp = P.spectral(Y, args.kClusters, seed=_seed(args), device=device)
    except ValueError as err:
        log.warning("--cluster SPECTRAL skipped: %s", err)
        return
    t = sp.timings
    log.info("SPECTRAL of %s points: cluster sizes %s; eigenvalues %s, %s iterations (residual %.3g), %s isolated; affinity %.1f ms, "
             "normalise %.1f ms, products %.1f ms (device) + %.1f ms (host), k-means %.1f ms", len(sp.labels),
             np.bincount(sp.labels).tolist(), sp.eigenvalues.tolist(), sp.n_iter, float(sp.residuals.max()), sp.n_isolated,
             t["affinity_ms"], t["normalise_ms"], t["products_ms"], t["host_ms"], t["kmeans_ms"])
    if args.dumpPCAdata:
        with open(os.path.join(args.tempDir, "anomSPECTRAL"), "wb") as fh:
            pickle.dump(sp.labels, fh, protocol=2)
    clock.lap("SPECTRAL")


def _spiked_counts(args, table, logKLD, threshold, feats, querySeq, device, clock):
    """--runProjection with --spikeNormal (the reference advertises the option as a future function and never wired it): the
    projection's input with ordinary windows beside the anomalies.  The query is loaded by the native reader and stays packed on
    the device; the vectors of the anomaly set and of the spiked windows (postprocess.spike_rows: as many as there are anomalies,
    nearest the median log10(KLD)) come from ONE projection.windowVectors call on it.  Returns (labelled, anomLabels, anomCounts,
    spiked): the anomaly rows first, order and labels as without the option, then the spiked rows labelled name:start:stop as the
    table reports them; spiked = the bool mask of the latter, None when there is nothing to spike."""
    from .engine import Engine
    from .projection import windowVectors
    with Engine(args.pcaMin, args.pcaMax, device) as e:
        index = {nm: i for i, nm in enumerate(e.load_fasta(querySeq))}
        lens = list(e.seq_lens)

        def ranges(records):        # (name, 1-based start, stop) -> what the slice seq[start - 1:stop] covers
            out = []
            for nm, a, b in records:
                lo, hi, _ = slice(int(a) - 1, int(b)).indices(lens[index[nm]])
                out.append((index[nm], lo, hi))
            return out
        anom = [(f[0], f[1], f[2]) for f in feats if f[0] in index]
        labelled = [":".join([nm, str(a), str(b)]) for nm, a, b in anom]
        rows = np.zeros(0, dtype=np.int64)
        if not anom:
            log.info("--spikeNormal: no anomalous window to set ordinary windows beside.")
        else:
            rows = pp.spike_rows(logKLD, pp.pickedKLD(logKLD, threshold, bool(args.findSelf)), len(anom))
            rows = rows[np.array([table.names[int(table.seq_index[r])] in index for r in rows.tolist()], dtype=bool)]
            if rows.size == 0:
                log.info("--spikeNormal: every scored window is anomalous or unscored: no ordinary window to add.")
        spikes = [(table.names[int(table.seq_index[r])], int(table.start[r]), int(table.stop[r])) for r in rows.tolist()]
        labels = labelled + [":".join([nm, str(a), str(b)]) for nm, a, b in spikes]
        where = ranges(anom + spikes)
        counts = windowVectors(e, [w[0] for w in where], [w[1] for w in where], [w[2] for w in where], args.pcaMin, args.pcaMax,
                               labels=labels)
    if spikes:
        log.info("--spikeNormal: %s ordinary windows nearest the median log10(KLD) beside %s anomalous ones.", len(spikes), len(anom))
    clock.lap("k-mer vectors (--spikeNormal)")
    spiked = np.arange(len(labels)) >= len(anom) if spikes else None
    return labelled, np.array([[lab] for lab in labels]) if labels else np.zeros((0, 1), dtype=object), counts, spiked


def _gff_features(args, anomalies, intervals):
    """--gffIn (L1709-1747): the records of the annotation whose type is in --gffFeatures and that lie within --gffRange bases of
    an anomaly (with a threshold option) or of a State1 / State2 interval of the main HMM track (--hmmKLD; `intervals` as hmm2BED
    returns them, with the coordinates their GFF carries), one file each, written only when a record is kept."""
    if not args.gffFeatures:
        log.info("--gffIn %s is not used: name the feature types to report with --gffFeatures.", args.gffIn)
        return
    records = pp.read_gff(args.gffIn, args.gffFeatures)
    base = os.path.basename(args.gffIn)

    def report(regions, stem, found, none):
        kept = pp.featuresNear(records, regions, args.gffRange)
        if kept:
            with open(os.path.join(args.tempDir, stem + base), "w") as fh:
                fh.writelines(kept)
            log.info("Successfully extracted %s features from within %sbp of %s annotations.", len(kept), args.gffRange, found)
        else:
            log.info("No features from %s detected within %s bases of %s.", args.gffIn, args.gffRange, none)
    if args.threshTypeKLD or args.forceThresholdKLD:
        report(anomalies, "featuresIn_thresholded_Anomalies_", "anomaly", "anomalies")
    if args.hmmKLD:
        for state in ("State1", "State2"):          # (the reference's filter is `type in 'State1'`; hmmBED2GFF writes these two types)
            report(pp.gffRegions(intervals, state), "featuresIn_hmm_%s_" % state, state + " hmm", state + " hmm features")


def _main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(funcName)s - %(message)s")
    args = mainArgs(argv)
    clock = _Clock()
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # the sharded code path can be forced in a one-rank job (tests rehearse it on a single GPU)
    sharded = world > 1 or os.environ.get("FRISK_FORCE_SHARDED") == "1"
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # FRISK_DIST_REHEARSAL=1: the N-rank job on ONE GPU - every rank on device 0, gloo instead of RCCL (which refuses two ranks
    # on one device): a functional rehearsal of the sharded path (tiles, all-reduce, row gather) where only one GPU exists
    rehearsal = os.environ.get("FRISK_DIST_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    if sharded and not dist.is_initialized():
        import torch
        torch.cuda.set_device(local_rank)
        if world == 1:      # FRISK_FORCE_SHARDED outside a launcher: a one-rank rendezvous of our own
            for key, val in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29517"), ("RANK", "0"), ("WORLD_SIZE", "1")):
                os.environ.setdefault(key, val)
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if rank == 0:
        print("frisk --", pp.FRISK_VERSION)
    genomepickle = makePicklePath(args, "genome")
    windowsPickle = makePicklePath(args, "window")
    querySeq = args.querySeq or args.hostSeq
    if rank == 0 and not os.path.isdir(os.path.abspath(args.tempDir)):
        os.makedirs(os.path.abspath(args.tempDir))
    if sharded:
        dist.barrier()      # tempDir exists, and every rank sees the same cache files, before anyone looks for them
    projection = args.runProjection in PROJECTIONS            # a projection this build runs and clusters
    clustering = projection and args.cluster in CLUSTERINGS
    # NMF runs, but every file written under --runProjection NMF before it was built stays as it was: the merged anomalies in
    # --gffOutfile and no cluster GFF3.  Both follow PROJECTIONS, so moving "NMF" there switches them together.
    projected_only = args.runProjection in PROJECTIONS_UNCLUSTERED + PROJECTIONS_DUMPED
    for opt, why in unavailable(args):
        log.warning("--%s is not available in this build: %s", opt, why)
    update = bool(args.updateHMM)
    if update and (sharded or args.exitAfter):
        log.warning("--updateHMM skipped: %s.", "a sharded job keeps tiles cut for the main window and increment" if sharded
                    else "--exitAfter %s stops before the features" % args.exitAfter)
        update = False
    fine_table = None

    from .hotpath import HotPath
    from . import distributed as D
    columns = _columns(args)
    rip = len(columns) == 8
    w, inc, all_ = args.windowlen, args.increment, bool(args.scaffoldsAll)
    # (the packed-sequence cache lives beside the pickle caches; --recalc - store_false - means: recompute, so rewrite it too)
    hp = HotPath(args.minWordSize, args.maxWordSize, device=local_rank, cache_dir=None if sharded else args.tempDir,
                 use_cache=bool(args.recalc))
    clock.lap("startup (imports + HIP context)")
    table = None
    index_writers = []
    out_threads, out_err = [], []           # the score table text and the window cache on their way to disk

    def _join_outputs():
        for th in out_threads:
            th.join()
        del out_threads[:]
        if out_err:
            raise out_err.pop(0)

    def _bg(fn, *a):
        import threading

        def run():
            try:
                fn(*a)
            except BaseException as err:        # noqa: B902 - re-raised on the main thread (_join_outputs)
                out_err.append(err)
        th = threading.Thread(target=run, name="frisk-" + fn.__name__)
        th.start()
        out_threads.append(th)

    def _write_genome_pickle(arrays):
        # the reference's pickled form (list of dicts + 3 metadata dicts, L356-359): 87 380 dict entries at K = 8, built and written
        # beside the scan, which needs only the profile on the device
        from .hotpath import profileToMaps
        maps = profileToMaps(arrays[0], arrays[1], arrays[2], arrays[3], args.minWordSize, args.maxWordSize)
        tmp = genomepickle + ".tmp%d" % os.getpid()
        with open(tmp, "wb") as fh:
            pickle.dump(maps, fh, protocol=2)
        os.replace(tmp, genomepickle)

    # Sharded jobs: a rank with a seek index of the FASTA (fasta_index.h; in --tempDir, or beside the file) copies the bytes of
    # its tiles instead of parsing all of it.  --recalc (store_false: recompute) ignores every index; where a rank had to
    # parse, rank 0 writes the index beside the other caches for the next run - in the background, it is not needed by this one.
    def _shard_index(fasta):
        from .fasta import fastaIndexPaths
        paths = fastaIndexPaths(fasta, args.tempDir)
        return paths if args.recalc else []         # (--recalc: no index at all, not ours and not a foreign <fasta>.fai)

    def _note_shard_load(fasta):
        if hp.engine.shard_index is not None:
            log.info("Read this rank's tiles of %s through the index %s", fasta, hp.engine.shard_index)
        elif rank == 0:
            import threading
            from .fasta import fastaIndexPaths, writeFastaIndex

            def _write(src=fasta, dst=fastaIndexPaths(fasta, args.tempDir)[0]):
                try:
                    writeFastaIndex(src, dst)
                except Exception as err:            # (a read-only --tempDir, a vanished file: the next run parses again)
                    log.info("No seek index written for %s: %s", src, err)
            th = threading.Thread(target=_write, name="frisk-fasta-index", daemon=True)
            th.start()
            index_writers.append(th)

    try:
        # ---- phase A: host k-mer profile (L1436-1447); --recalc is store_false: giving it forces recomputation.
        # Under torchrun every rank takes the same branch (the cache is a file all ranks see); rank 0 writes it.
        resident_names = None       # sharded: names of the FASTA whose tiles are resident
        if os.path.isfile(genomepickle) and args.recalc:
            log.info("Importing previously calculated genome kmers from %s", genomepickle)
            with open(genomepickle, "rb") as fh:
                genomeKmers = pickle.load(fh, encoding="latin1")
            hp.setGenomeProfile(genomeKmers)
            clock.lap("profile cache")
        else:
            log.info("Calculating kmers for host sequence: %s", args.hostSeq)
            if sharded:
                resident_names = D.profile_sharded(hp.engine, args.hostSeq, w, inc, mask_host=args.maskHost, scaffolds_all=all_,
                                                   index=_shard_index(args.hostSeq))
                _note_shard_load(args.hostSeq)
                profile_arrays = hp.engine.profile_get() if rank == 0 else None
            else:
                hp._load(args.hostSeq)
                clock.lap("packed sequence cache -> HBM" if hp.loaded_from_cache else "FASTA parse + upload + pack")
                profile_arrays = hp.genomeProfileArrays(args)
            clock.lap("phase A (profile)" if not sharded else "phase A (parse + upload + profile + all-reduce)")
            if rank == 0:
                _bg(_write_genome_pickle, profile_arrays)               # (joined with the other outputs, or right below)
            if args.exitAfter == "GenomeKmers":                          # L1443-1445: before any window is scored
                _join_outputs()
                clock.lap("profile pickle")
                log.info("Finished counting kmers. Exiting.")
                return 0
        # ---- phase B: window scores (L1454-1507)
        if os.path.isfile(windowsPickle) and args.recalcWin:
            log.info("Importing previously calculated window KLD scores from: %s", windowsPickle)
            if rank == 0:
                table = _load_window_cache(windowsPickle, rip)
            clock.lap("window cache")
        else:
            zero = None
            try:
                if sharded:
                    same = querySeq == args.hostSeq and resident_names is not None
                    table, failed = D.scan_sharded(hp.engine, querySeq, w, inc, rip=rip, scaffolds_all=all_,
                                                   resident_names=resident_names if same else None, index=_shard_index(querySeq))
                    if not same:
                        _note_shard_load(querySeq)
                    if failed:
                        zero = ZeroDivisionError("float division by zero")          # on EVERY rank (L437)
                else:
                    table, _res = hp.scanTable(args, querySeq)
            except ZeroDivisionError as err:
                zero, table = err, getattr(err, "table", None)
            clock.lap("phase B (scan)")
            if rank == 0 and table is not None:
                if zero is None:
                    # Two files of the same rows - the window cache (L1501) and the table text (native formatter, outside the
                    # interpreter lock), neither reads the other - written in the background while thresholds, segmentation and
                    # features are computed from the same (read-only) columns; joined before this function returns or raises.
                    _bg(_dump_window_cache, windowsPickle, table)
                    _bg(write_table, os.path.join(args.tempDir, args.outfile), table)
                else:
                    # the reference writes and prints row by row (L1487-1494): what it had written before dying is written here too
                    write_table(os.path.join(args.tempDir, args.outfile), table)
                clock.lap("score table text + window pickle started" if zero is None else "score table text")
            if zero is not None:
                raise zero
        if update:              # before the HotPath is closed; loads the sequence where both caches were hit (the profile is set)
            fine_table = _fine_scan(args, hp, querySeq, clock)
    except BaseException:
        for th in out_threads:
            th.join()
        raise
    finally:
        for th in index_writers:
            th.join()
        hp.close()
    if rank != 0:
        return 0
    if args.exitAfter == "WindowKLD":
        _join_outputs()
        clock.lap("score table text + window pickle written")
        log.info("Finished calculating window KLD scores. Exiting.")
        clock.report()
        return 0

    try:
        # ---- thresholds and features (L1522-1530, L1671-1707)
        kld = np.where(table.kld_is_int0 != 0, 0.0, table.kld)
        with np.errstate(divide="ignore"):
            logKLD = np.log10(kld.reshape(-1, 1))
        threshold, _bins = pp.setKLDThresh(args, logKLD)
        threshold = float(np.ravel(threshold)[0])
        log.info("log10(KLD) threshold = %s", threshold)
        clock.lap("KLD threshold")
        if args.hmmKLD:                                                     # L1537-1548
            from .hmm import hmm2BED, hmmBED2GFF
            intervals, _model = hmm2BED(table)
            with open(os.path.join(args.tempDir, args.hmmOutfile), "w") as fh:
                fh.writelines(hmmBED2GFF(intervals))
            log.info("HMM segmentation: %s state features (fit: %s EM rounds, log-likelihood %s)", len(intervals),
                     getattr(_model, "n_iter_", "?"), getattr(_model, "loglik_", "?"))
            clock.lap("HMM segmentation + GFF")
        fine_intervals = None
        spiked = None               # --spikeNormal: which rows of the projection's input are spiked windows (None: no spikes)
        if args.spikeNormal and not args.runProjection:
            log.warning("--spikeNormal has no effect without --runProjection.")
        if fine_table is not None:                                          # --updateHMM: the fine track, device model
            from .hmm import hmm2BED, hmmBED2GFF
            if not np.any(~np.isnan(np.where(fine_table.kld_is_int0 != 0, 0.0, fine_table.kld))):
                log.warning("--updateHMM skipped: the fine scan (-w %s -i %s) scored no window.", args.updateWin, args.updateInc)
            else:
                fine_intervals, fmodel = hmm2BED(fine_table, _fine_model(local_rank))
                with open(os.path.join(args.tempDir, fineTrackName(args)), "w") as fh:
                    fh.writelines(hmmBED2GFF(fine_intervals))
                log.info("Fine HMM track (-w %s -i %s, %s windows): %s state features (fit: %s EM rounds, log-likelihood %s)",
                         args.updateWin, args.updateInc, len(fine_table), len(fine_intervals), fmodel.n_iter_, fmodel.loglik_)
            clock.lap("fine HMM segmentation + GFF (--updateHMM)")
        if args.runProjection:                                              # L1556-1596: counts for the projection
            from .fasta import readFasta
            from .projection import symmetricCounts
            feats, _ = pp.thresholdKLD(table, threshold, args, merge=(args.dimReduce == "features"))
            if args.spikeNormal:
                labelled, anomLabels, anomCounts, spiked = _spiked_counts(args, table, logKLD, threshold, feats, querySeq, local_rank, clock)
            else:
                names, seqs = readFasta(querySeq)
                fasta = dict(zip(names, seqs))
                labelled = [(":".join([f[0], str(f[1]), str(f[2])]), fasta[f[0]][int(f[1]) - 1:int(f[2])]) for f in feats if f[0] in fasta]
                anomLabels, anomCounts = symmetricCounts(labelled, args.pcaMin, args.pcaMax, device=local_rank)
            if args.dumpPCAdata:
                with open(os.path.join(args.tempDir, "anomLabels"), "wb") as fh:
                    pickle.dump(anomLabels, fh, protocol=2)
                with open(os.path.join(args.tempDir, "anomCounts"), "wb") as fh:
                    pickle.dump(anomCounts, fh, protocol=2)
                if spiked is not None:
                    with open(os.path.join(args.tempDir, "anomSpike"), "wb") as fh:
                        pickle.dump(spiked, fh, protocol=2)
            if projection or projected_only:
                y_pred = _project(args, anomCounts, local_rank, clock)
            else:
                log.info("Symmetric k-mer proportions of %s anomalous windows computed; the %s projection is not built here.",
                         len(labelled), args.runProjection)
        if projection:
            anomalies = feats           # L1672-1675: the projection's own anomaly set (single windows under --dimReduce windows)
        else:
            anomalies, _sel = pp.thresholdKLD(table, threshold, args, merge=True)
        log.info("Detected %s features above KLD threshold.", len(anomalies))
        if args.gffOutfile:
            with open(os.path.join(args.tempDir, args.gffOutfile), "w") as fh:
                for line in pp.anomaly2GFF(anomalies, args):
                    fh.write(line)
            if fine_intervals is not None:                                  # --updateHMM: the same set, boundaries refined
                refined, _kept = pp.refineAnomalies(fine_intervals, anomalies)
                with open(os.path.join(args.tempDir, "HMMupdated_" + args.gffOutfile), "w") as fh:
                    fh.writelines(pp.anomaly2GFF(refined, args))
            if clustering:                                                  # L1688-1697
                rows = pp.cluster_rows(anomLabels, y_pred)
                if spiked is not None:      # --spikeNormal: the anomalies keep their file, with the classes of the joint clustering
                    with open(os.path.join(args.tempDir, "spikeNormal_" + pp.clusterGffName(args)), "w") as fh:
                        fh.writelines(pp.anomClust2gff([r for r, s in zip(rows, spiked) if s]))
                    rows = [r for r, s in zip(rows, spiked) if not s]
                with open(os.path.join(args.tempDir, pp.clusterGffName(args)), "w") as fh:
                    fh.writelines(pp.anomClust2gff(rows))
        if rip:
            feats = pp.thresholdRIP(table, args)
            if feats:
                with open(os.path.join(args.tempDir, args.RIPgff), "w") as fh:
                    for line in pp.RIP2GFF(feats):
                        fh.write(line)
            else:
                log.info("No RIP features detected.")
        clock.lap("anomaly / RIP features + GFF")
        if args.gffIn:                                                      # L1709-1747
            _gff_features(args, anomalies, intervals if args.hmmKLD else None)
            clock.lap("gffIn features")
    except BaseException:
        for th in out_threads:           # (the two output files are finished before the error travels on)
            th.join()
        raise
    _join_outputs()
    clock.lap("score table text + window pickle written")
    clock.report()
    return 0
