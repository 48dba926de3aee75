/* frisk_hip.h - C ABI of libfrisk_hip.so: the MI355X (gfx950) implementation of frisk's hot path.
 *
 * The reference (Adamtaranto/frisk, one Python-2 module) has no FFI, plugin or operator
 * interface; its only stable boundary is the call pattern inside main().  Each entry point
 * below names the reference lines it replaces (citations are to /root/reference/frisk/__init__.py):
 *
 *   phase A  genome k-mer profile      computeKmers(genomeMode=True)   L1442  (L280-367)
 *   phase B  window scan               the loop L1478-1494: crawlGenome (L194-251) ->
 *            computeKmers(window) (L280-367) -> IvomBuild x2 (L369-457) -> KLD (L459-472)
 *            -> calcGC (L120-137) [-> calcRIP (L474-495)]
 *
 * Conventions: plain C, plain pointers and sizes, no exceptions, no torch types.  Every
 * function returning int returns FRISK_OK (0) or a negative FRISK_E_* code; the message is
 * available from frisk_last_error().  The caller owns every host buffer it passes; the
 * library never keeps a caller pointer after the call returns.  A context is bound to one
 * device and one HIP stream and is not thread-safe; use one context per device per thread
 * (multi-GPU = one process per GPU, one context each).  K-mer index convention (reference
 * L70, L253-274): digits A=0,T=1,G=2,C=3, first base most significant; tables for orders
 * kmin..kmax are concatenated in ascending order ("profile layout", frisk_profile_len()).
 */
#ifndef FRISK_HIP_H
#define FRISK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frisk_ctx frisk_ctx;

enum {
    FRISK_OK = 0,
    FRISK_E_ARG = -1,         /* bad argument / unsupported geometry                                   */
    FRISK_E_HIP = -2,         /* a HIP runtime call failed (no device, out of memory, launch failure)  */
    FRISK_E_STATE = -3,       /* call order violated (e.g. scan before a profile is finalised)         */
    FRISK_E_CAP = -4,         /* caller buffer too small; the needed size is reported                  */
    FRISK_E_ZERO_WEIGHT = -5, /* reserved: ZeroDivisionError cases are reported per row (FRISK_ROW_ZERO_WEIGHT)  */
    FRISK_E_INDEX = -6        /* no usable seek index for this FASTA file: the caller parses it instead  */
};

/* frisk_scan flags */
#define FRISK_SCAN_RIP           1u   /* fill pi/si/cri (--RIP, L1485-1486); needs kmin <= 2 <= kmax  */
#define FRISK_SCAN_SCAFFOLDS_ALL 2u   /* --scaffoldsAll: small scaffolds become one window (L211-221) */
#define FRISK_SCAN_CHUNKS       256u /* schedule the windows in chunks of 8 consecutive candidates whatever the scan's size (a short
                                        scan is otherwise dealt window by window): the path long scans take - tables sliding from
                                        window to window inside a chunk - on inputs of any size.  Results are the same bits. */
#define FRISK_SCAN_BITS4        512u /* K = 8: the bulk launch with 4-bit counters whatever the scan's size, overflowing windows handed on
                                        to the 8- and 16-bit forms (a short scan otherwise starts at 8 bits; a long one samples first).
                                        Results are the same bits. */
#define FRISK_SCAN_SIDE4       1024u /* K = 8: as FRISK_SCAN_BITS4, with the side table for the max-mers of period <= 4 (poly-A, (CA)n, (AAAT)n
                                        ...) beside the 4-bit counters - the form a long scan of repeat-rich sequence picks by itself.
                                        Results are the same bits. */
#define FRISK_SCAN_GENERIC     2048u /* K = 8, lowest order 1: the 4-bit bulk launch keeps the kernel that reads the lowest order as an argument
                                        instead of the one compiled for 1 (what such a scan otherwise takes).  Results are the same bits. */

/* per-row status bits written to `status` by frisk_scan */
#define FRISK_ROW_KEPT        1u      /* window passed the < 30 % non-ACGT filter (L237-241)          */
#define FRISK_ROW_ZERO_WEIGHT 2u      /* reference raises ZeroDivisionError for this window (kld = NaN) */
#define FRISK_ROW_JUMPBACK    4u      /* end-of-scaffold "jumpback" window (0-based start, L230-243)  */
#define FRISK_ROW_NO_MAXMER   8u      /* no valid max-mer: the reference's KLD is the int 0 (L465)    */

const char* frisk_version(void);

/* Library limits for (kmin,kmax,window length); 0 = unsupported.  kmax <= 12 (the reference's -k is unbounded, L1197-1206,
 * but its own cost grows with 4^K); kmax <= 8 and windows up to 65535 bases run in LDS, everything else (windows up to
 * 2^31-1 bases, kmax 9..12) on a slower path with 32-bit tables in global memory. */
int frisk_supported(int kmin, int kmax, int64_t max_window);

/* Context: device ordinal, word sizes -m/-k (L1197-1206). */
int  frisk_create(int device, int kmin, int kmax, frisk_ctx** out);
void frisk_destroy(frisk_ctx* ctx);
const char* frisk_last_error(const frisk_ctx* ctx);   /* library-owned, valid until the next call on ctx */
int64_t frisk_profile_len(const frisk_ctx* ctx);      /* sum_{x=kmin..kmax} 4^x                          */

/* ---- sequence residency ------------------------------------------------------------------
 * Replaces the hand-off of scaffold strings from iterFasta (L139-164) to the counters
 * (L297, L203).  Uploads n_seq scaffolds (ASCII, any case, any IUPAC letter), packs them on
 * the device to 2 bits/base + validity and soft-mask bitmaps, and keeps them resident until the
 * next load.  Empty scaffolds (len 0) are allowed.  A refused load (FRISK_E_ARG: n_seq < 0, a negative length) changes nothing:
 * the resident batch, its lengths and names stay as they were.  The same holds for frisk_seq_synth / frisk_seq_synth2. */
int frisk_seq_load(frisk_ctx* ctx, const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq);

/* Double-buffered residency - the "streamed to HBM" of the north star.  frisk_seq_stage uploads and packs the NEXT batch on
 * a second HIP stream while the resident batch is being profiled / scanned; frisk_seq_commit makes it the resident batch
 * (the compute stream waits for the upload on the device, the host does not block).  The copies are asynchronous when the
 * source buffers are page-locked (frisk_host_alloc); the caller keeps them alive until the next call after the commit that
 * synchronises with the device - frisk_scan, frisk_profile_get, frisk_profile_export_host, frisk_seq_export_packed,
 * frisk_seq_read (frisk_profile_reset / _add / _finalize only enqueue).  A stage also waits, on the device, for work
 * queued before the last commit: the slot it fills may still be read by that work.  frisk_seq_stage_packed takes the three bit-packed arrays in the
 * library's own layout (as frisk_seq_export_packed returns them for the same `lens`): 0.5 bytes per base over PCIe instead
 * of 1, and no parsing - the sequence-cache path of the CLI. */
int frisk_seq_stage(frisk_ctx* ctx, const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq);
int frisk_seq_stage_packed(frisk_ctx* ctx, const uint32_t* codes, const uint32_t* inv, const uint32_t* low,
                           const int64_t* lens, int32_t n_seq);
/* The 0.25 B/base upload form - the north star's "2-bit-packed and streamed to HBM", SURVEY.md 8(d)'s algorithmic bytes: only
 * the 2-bit codes travel densely (2 * P / 32 words, P = frisk_padded_len_of(lens, n_seq), library layout: scaffold s at padded
 * positions [off, off + len), one PAD behind it, 16 bases per word, first base most significant); the two masks travel as run
 * lists - n_inv / n_low pairs [begin, end) of padded positions, ascending and disjoint: inv = letters other than ACGTacgt,
 * low = lowercase acgt - and are expanded to the bitmaps on the device; PADs are the library's business.  n_inv (n_low) < 0:
 * the argument is the dense bitmap instead (P / 32 words, PAD bits clear) - for an assembly with more runs than bitmap words.
 * The codes cross PCIe in pieces of piece_bases positions (0: the library's default, 256 Mbases = 64 MB) with an event behind
 * each: frisk_seq_commit does not wait for them, and frisk_profile_add(-1, -1) on the committed batch counts piece i while
 * piece i + 1 is on its way, so that of phase A only the last piece's kernel follows the upload.  Any other use of the batch
 * waits (on the device) for the last piece - a load that replaces the batch in its slot included.  Replaces, with frisk_pack_2bit, the hand-off of scaffold strings from iterFasta
 * (L139-164) to computeKmers (L297) and crawlGenome (L203).  Caller keeps the arrays alive as for frisk_seq_stage. */
int frisk_seq_stage_2bit(frisk_ctx* ctx, const uint32_t* codes, const int64_t* inv_runs, int64_t n_inv, const int64_t* low_runs,
                         int64_t n_low, const int64_t* lens, int32_t n_seq, int64_t piece_bases);
/* Host-only (multi-threaded): scaffolds as ASCII -> that form.  codes: caller's buffer of 2 * P / 32 words (page-locked memory
 * makes the upload asynchronous); *inv_runs / *low_runs: malloc'd by the library (frisk_free), n pairs each. */
int frisk_pack_2bit(const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq, uint32_t* codes, int64_t** inv_runs,
                    int64_t* n_inv, int64_t** low_runs, int64_t* n_low);
int64_t frisk_padded_len_of(const int64_t* lens, int32_t n_seq);   /* P: sum(len + 1) rounded up to 32 (32 for an empty batch); -1: bad lengths */
/* The resident batch in that form (the CLI's sequence cache): codes into the caller's buffer, run lists malloc'd (frisk_free). */
int frisk_seq_export_2bit(frisk_ctx* ctx, uint32_t* codes, int64_t** inv_runs, int64_t* n_inv, int64_t** low_runs, int64_t* n_low);
int frisk_seq_commit(frisk_ctx* ctx);
/* Packed arrays of the resident batch: codes 2 * P / 32 words, inv and low P / 32 words each, P = frisk_seq_padded_len(). */
int frisk_seq_export_packed(frisk_ctx* ctx, uint32_t* codes, uint32_t* inv, uint32_t* low);
/* Record names for a batch that did not come from frisk_fasta_load (e.g. from the sequence cache). */
int frisk_seq_set_names(frisk_ctx* ctx, const char* const* names, int32_t n_seq);

/* Native FASTA reader: parse `path` (plain or gzip) with the record semantics of the reference's iterFasta
 * (L139-164: name = first whitespace-delimited token of the header with '>' stripped from both ends, lines stripped of
 * surrounding whitespace, blank lines skipped, case preserved) straight into the upload layout, and make its records
 * the resident batch.  Record names / lengths are then available from frisk_seq_name / frisk_seq_len. */
int frisk_fasta_load(frisk_ctx* ctx, const char* path, int32_t* n_seq, int64_t* total_len);
/* Host-only test utility: parse `path` with the native reader and return the number of records, their total length and an
 * FNV-1a digest over (name, 0, sequence, 0) of every record - what the CPU test-suite compares with the Python reader. */
int frisk_fasta_digest(const char* path, int32_t* n_seq, int64_t* total_len, uint64_t* digest);
/* Host-only: a FASTA file (plain or gzip) straight into the 0.25 B/base form - what frisk_fasta_load does before its upload (iterFasta
 * L139-164 -> frisk_pack_2bit in one pass over the mapped file, no one-byte-per-base buffer in between).  All five arrays are
 * malloc'd by the library (frisk_free): *lens (n_seq values), *codes (*n_code_words = 2 * P / 32 words), the two run lists. */
int frisk_fasta_pack_2bit(const char* path, int32_t* n_seq, int64_t** lens, uint32_t** codes, int64_t* n_code_words, int64_t** inv_runs,
                          int64_t* n_inv, int64_t** low_runs, int64_t* n_low);

/* Multi-GPU form of frisk_fasta_load (window-tile sharding with halo): every rank parses the file, but keeps
 * resident only what it needs for ITS share of the job - the candidate windows [*cand_begin, *cand_end) of the job's
 * numbering (an equal contiguous share) and the positions whose k-mers it counts in phase A (every base of the genome
 * belongs to exactly one rank; K-1 bases of halo behind each owned range).  The window geometry is fixed here; frisk_scan
 * on the batch then numbers candidates from 0 = *cand_begin, frisk_profile_add(-1,-1) counts the owned positions, and
 * seq_index / frisk_seq_name / frisk_seq_len / frisk_seq_count refer to the records of the FASTA, as on one GPU. */
int frisk_fasta_load_shard(frisk_ctx* ctx, const char* path, int32_t w, int32_t inc, uint32_t flags, int32_t rank,
                           int32_t world, int32_t* n_seq, int64_t* total_len, int64_t* cand_begin, int64_t* cand_end);
/* The same without parsing the file: a seek index (frisk_amd/csrc/fasta_index.h: one `samtools faidx` line per record behind a
 * stamp line with the FASTA's size and modification time; a foreign <fasta>.fai that is not older than the file is accepted
 * too) tells the rank where the bases of ITS tiles are, and it copies those bytes from the mapped file - 1/world of the
 * file + halos instead of all of it.  The index is checked against the file where it is used (a header line that gives the
 * record's name ends right before its first base, its last base ends a line).  FRISK_E_INDEX: no usable index (missing,
 * made from another version of the file, gzip, a record the byte arithmetic cannot address) - call frisk_fasta_load_shard.
 * The reference reads every record of the file on every run (iterFasta, L139-164). */
int frisk_fasta_load_shard_indexed(frisk_ctx* ctx, const char* path, const char* index_path, int32_t w, int32_t inc,
                                   uint32_t flags, int32_t rank, int32_t world, int32_t* n_seq, int64_t* total_len,
                                   int64_t* cand_begin, int64_t* cand_end);
/* Host-only: write the seek index of `fasta_path` to `index_path` (one pass over the mapped file).  FRISK_E_INDEX when the
 * file is not regular - text before the first header, blank lines or surrounding blanks inside a record, lines of different
 * length before a record's last, gzip - with the reason in `why` (nullable). */
int frisk_fasta_index_build(const char* fasta_path, const char* index_path, int32_t* n_seq, char* why, int32_t why_cap);
/* Host-only test / extraction utility: bases [pos0, pos0 + n) of record seq_index through the index (seq_index < 0: the number
 * of records alone; n = 0: name and length alone).  Any output pointer may be NULL. */
int frisk_fasta_index_read(const char* fasta_path, const char* index_path, int32_t seq_index, int64_t pos0, int64_t n,
                           uint8_t* out, int32_t* n_seq, int64_t* seq_len, char* name, int32_t name_cap, char* why,
                           int32_t why_cap);
int32_t frisk_seq_count(const frisk_ctx* ctx);
const char* frisk_seq_name(const frisk_ctx* ctx, int32_t seq_index);   /* "" for batches not loaded from FASTA */
int64_t frisk_seq_len(const frisk_ctx* ctx, int32_t seq_index);

/* Bench/test utility: fill the resident batch with synthetic scaffolds generated ON the device
 * (order-3 Markov background + compositional islands + N runs + soft-masked runs + simple repeats - poly-A / poly-T
 * tails and microsatellites, repeats_per_kb of them per 1000 bases, soft-masked; the generator is specified in
 * frisk_amd/synth.py, which reproduces it bit-for-bit on the host). */
int frisk_seq_synth(frisk_ctx* ctx, const int64_t* lens, int32_t n_seq, uint64_t seed,
                    double island_frac, double n_frac, double lower_frac, double repeats_per_kb);
/* ... with repeat content no table of the scan kernel is shaped after: a share period_mix of the simple repeats is of period 3, 5
 * or 6 ((CAG)n, (AAT)n, (AAAAT)n, (TTAGGG)n, up to 210 bases), and a share sat_frac of the bases lies in satellite arrays - tandem
 * copies of a 171-base monomer, 3 % divergence between copies, 0.13 .. 1.05 Mb each (frisk_amd/synth.py is the specification). */
int frisk_seq_synth2(frisk_ctx* ctx, const int64_t* lens, int32_t n_seq, uint64_t seed, double island_frac, double n_frac,
                     double lower_frac, double repeats_per_kb, double period_mix, double sat_frac);

/* Null sequences: fill the resident batch with n_seq sequences drawn ON the device from the order-`order` Markov chain of the
 * context's FINALISED profile - context c in [0, 4^order) continues with base b in proportion to the symmetric count of the
 * (order + 1)-mer 4c + b (csrc/null_kernels.h; frisk_amd/nullmodel.py is the specification and reproduces the bytes on the host).
 * Uppercase A/T/G/C only.  Every base is a pure function of (profile, order, seed, sequence index, position): a sequence is a
 * prefix of any longer one of the same index.  The batch is laid out, packed and made resident as frisk_seq_synth2's, names "";
 * the scan plan is invalidated as by any new batch; the profile, the panel and every row buffer are left alone.
 * FRISK_E_ARG, with nothing launched and the resident batch as it was: order < 0, order + 1 outside kmin .. kmax, a null length
 * table, a negative length, n_seq < 0.  FRISK_E_STATE: no finalised profile.
 * frisk_last_kernel_ms(ctx, 6) = the generator kernels' time (table + draw) of the last call. */
int frisk_seq_null(frisk_ctx* ctx, const int64_t* lens, int32_t n_seq, uint64_t seed, int32_t order);

/* Copy bases [offset, offset+n) of resident scaffold seq_index back as ASCII (canonical letters:
 * A/T/G/C, a/t/g/c, N for every non-ACGT letter) - test / bench-sampling utility. */
int frisk_seq_read(frisk_ctx* ctx, int32_t seq_index, int64_t offset, int64_t n, uint8_t* out);

/* ---- k-mer proportion vectors of arbitrary ranges (the projection's input, L1573-1591) -------
 * Row r of X (n x F doubles on the host, F = number of reverse-complement-folded words of orders kmin..kmax: 2 772 for 1..6) is
 * the reference's computeKmers(sym=True, pcaMode=True) -> scrubMirrors -> flattenKmerMap(prop=True) vector (L280-367, L797-831) of
 * bases [start[r], stop[r]) - 0-based, half-open - of scaffold seq_index[r] of the resident batch, counted on the device from the
 * packed batch (csrc/kvec_kernels.h): lowercase counts, a word with a base outside ACGTacgt does not, and no word reaches past
 * stop[r].  nn[r] = the reference's countN of the range (positions that are not uppercase A/T/G/C); status[r] has
 * FRISK_KVEC_EMPTY_ORDER set when the range holds no valid word of some order, and bit FRISK_KVEC_ORDER_SHIFT + x for every such
 * order x (the row's entries of that order are then 0, never a division by zero).  kmin / kmax are independent of the context's
 * own orders: 1 <= kmin <= kmax <= FRISK_KVEC_MAX_K.  The rows are computed batch_rows at a time (0: as many as keep the
 * device-side block of X at or under 256 MB).  FRISK_E_ARG, with nothing launched: no resident batch, a tiled batch, an index out
 * of range, start < 0, stop <= start, stop > frisk_seq_len, a range of 2^32 bases or more, orders outside the above.  n = 0 is
 * FRISK_OK and touches no output.  frisk_last_kernel_ms(ctx, 3) = the kernels' time, summed over the batches of the last call. */
#define FRISK_KVEC_MAX_K 7
#define FRISK_KVEC_THREADS 256          /* one workgroup per range */
#define FRISK_KVEC_GRID_CAP 2048        /* workgroups of one launch: further ranges by grid stride */
#define FRISK_KVEC_EMPTY_ORDER 1u
#define FRISK_KVEC_ORDER_SHIFT 8        /* status bit 8 + x: order x is the empty one */
int frisk_window_vectors(frisk_ctx* ctx, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n, int kmin,
                         int kmax, int64_t batch_rows, double* X, int64_t* nn, uint32_t* status);

/* ---- phase A: genome profile (computeKmers genomeMode=True, L1442) -------------------------
 * reset -> add (once per resident batch; forward counts only) -> [all-reduce across GPUs]
 * -> finalize (adds the reverse complement, L350-351, and builds the genome-side IVOM table). */
int frisk_profile_reset(frisk_ctx* ctx);
/* Count the k-mers that START in padded positions [pos_begin,pos_end) of the resident batch;
 * pos_begin = pos_end = -1 means the whole batch.  mask_host: bit 0 = --maskHost (L336-337); bit 1 = FRISK_PROFILE_ONE_PASS, a test
 * hook: at kmax = 8 take the one-pass form with 16-bit LDS counters (what ranges of 2^30+ positions take by themselves; a wrapped
 * counter falls back to the two-pass form) whatever the size; at other kmax it changes nothing.  Same counts either way: bit 1 never
 * masks, on any path (kmax > 8, a streamed batch counted piece by piece, a tiled batch). */
#define FRISK_PROFILE_ONE_PASS 2
int frisk_profile_add(frisk_ctx* ctx, int mask_host, int64_t pos_begin, int64_t pos_end);
int64_t frisk_seq_padded_len(const frisk_ctx* ctx);
/* Raw (linear, summable) profile state: int64[frisk_profile_raw_len()] on the device.  To
 * all-reduce across GPUs the caller exports it into its own device buffer (e.g. a torch
 * tensor), runs ONE RCCL all-reduce(sum) on that, and imports the result. */
int64_t frisk_profile_raw_len(const frisk_ctx* ctx);
int frisk_profile_export_device(frisk_ctx* ctx, void* dst_device_int64);
int frisk_profile_import_device(frisk_ctx* ctx, const void* src_device_int64);
/* The same without copies and without the host: *raw = the raw profile's own device buffer (int64[frisk_profile_raw_len()]),
 * *stream = the context's HIP stream (a hipStream_t).  A collective library sums the buffer IN PLACE ON THAT STREAM - RCCL's
 * all-reduce over xGMI, issued under torch.cuda.ExternalStream(*stream) - so that profile_add -> all-reduce -> finalize is
 * one chain of enqueued work.  The call marks the profile as changed (as frisk_profile_import_device does). */
int frisk_profile_device_view(frisk_ctx* ctx, void** raw, void** stream);
/* The one exchange step of a multi-GPU job without any framework: RCCL all-reduce(sum, int64) of the raw profile
 * IN PLACE over `rccl_comm` (an ncclComm_t of the caller's making: one rank per GPU, created with ncclCommInitRank on this
 * context's device), enqueued on the context's stream - profile_add -> all-reduce -> finalize stay one chain, the host does
 * not wait.  rccl_comm = NULL: a single GPU, nothing to do.  librccl is resolved at first use (the instance already in the
 * process if there is one); it is not a link-time dependency of the library. */
int frisk_profile_allreduce(frisk_ctx* ctx, void* rccl_comm);
int frisk_profile_export_host(frisk_ctx* ctx, int64_t* dst_host);
int frisk_profile_import_host(frisk_ctx* ctx, const int64_t* src_host);
int frisk_profile_finalize(frisk_ctx* ctx);
/* The finished profile in the reference's terms: symmetric counts in profile layout and the
 * three metadata values of L356-359.  Any output pointer may be NULL. */
int frisk_profile_get(frisk_ctx* ctx, int64_t* sym_counts, int64_t* total_len, int64_t* ex_max,
                      int64_t* nn_total);
/* Install a finished profile (e.g. from a cache file; replaces pickle.load at L1437-1439). */
int frisk_profile_set(frisk_ctx* ctx, const int64_t* sym_counts, int64_t total_len, int64_t ex_max,
                      int64_t nn_total);

/* ---- phase B: window scan (loop L1478-1494) -------------------------------------------------
 * Candidate windows of the resident batch are numbered in output order (scaffold order, then j
 * ascending, L228); frisk_scan_plan returns their number.  frisk_scan scores candidates
 * [c0,c1) (c1 = -1: to the end) and writes one entry per candidate, index (c - c0); entries
 * whose status lacks FRISK_ROW_KEPT are windows the reference drops (no row).  cap = length of
 * the output arrays (FRISK_E_CAP if < c1-c0).  Nullable: pi/si/cri (required with
 * FRISK_SCAN_RIP), dbg_counts (cap x frisk_profile_len() uint32: the window's k-mer counts),
 * dbg_meta (cap x 3: totalLen, exMax, nnTotal of L356-359). */
int frisk_scan_plan(frisk_ctx* ctx, int32_t w, int32_t inc, uint32_t flags, int64_t* n_candidates);
int frisk_scan(frisk_ctx* ctx, int32_t w, int32_t inc, uint32_t flags, int64_t c0, int64_t c1,
               int64_t cap, int32_t* seq_index, int64_t* start, int64_t* stop, uint32_t* status,
               double* kld, double* gc, double* pi, double* si, double* cri,
               uint32_t* dbg_counts, int64_t* dbg_meta);

/* ---- the scan loop's columns of arbitrary ranges -------------------------------------------
 * Row r is one iteration of the scan loop (L1478-1494: computeKmers(window), both IvomBuilds, KLD, calcGC, calcRIP) on bases
 * [start[r], stop[r]) - 0-based, half-open - of scaffold seq_index[r] of the resident batch, against the context's finalised
 * profile and orders: a merged anomaly, a refined boundary, a gene, or - with another genome's profile in the context - the
 * same regions against a donor.  The range is scored as the slice it is (as frisk_window_vectors counts it): no word reaches past
 * stop[r], lowercase counts in words, S = its uppercase A/C/G/T.  One workgroup per range (csrc/range_kernels.h): 16-bit tables
 * in LDS for kmax <= 8 and ranges up to 65 535 bases, 32-bit tables in global scratch otherwise; a row's bits depend on the range
 * and the profile alone - not on the other rows, their order, the form or the grid.
 * status[r]: the FRISK_ROW_* bits (FRISK_ROW_JUMPBACK is never set); nn[r] = length - S, always written.  A range with
 * nn >= 0.3 * length is left unscored as the reference leaves such a window (L238): no FRISK_ROW_KEPT, NaN in every double
 * column.  FRISK_ROW_NO_MAXMER: kld = 0.  FRISK_ROW_ZERO_WEIGHT (a max-mer present and kmin-1 <= S <= kmax-1, or a max-mer without
 * genome weight, as in frisk_scan): kld = NaN.  Ranges with S < kmin-1 (negative divisors) are unspecified, as in frisk_scan.
 * flags: FRISK_SCAN_RIP fills pi/si/cri (nullable otherwise; needs kmin <= 2 <= kmax, else FRISK_E_ARG); FRISK_RANGES_BIG is a
 * test hook that forces the global-scratch form on every range (the same bits).
 * FRISK_E_ARG, with nothing launched: no resident batch, a tiled batch, an index out of range, start < 0, stop <= start,
 * stop > frisk_seq_len, a range of 2^31 bases or more, a null required array.  FRISK_E_STATE: no finalised profile.  n = 0 is
 * FRISK_OK and touches no output.  A streamed batch is waited for.  The scan's plan and rows are left alone.
 * frisk_last_kernel_ms(ctx, 4) = the kernels' time of the last call. */
#define FRISK_RANGES_BIG 0x10000u
int frisk_score_ranges(frisk_ctx* ctx, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                       uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri,
                       int64_t* nn);

/* ---- the same rows against a panel of genome profiles, in one pass ---------------------------
 * "Where did this region come from?" asked of many candidate donors at once.  A context keeps a PANEL of finalised genome-side
 * tables on the device; frisk_score_ranges_panel counts each range once and scores it against every profile of the panel
 * (csrc/panel_kernels.h).
 * frisk_panel_push appends a SNAPSHOT of the context's finalised genome-side table and returns its index in *slot (nullable).
 *   The panel holds a copy: frisk_profile_reset / _set / _finalize never change a stored slot afterwards, and the panel never
 *   changes the context's own profile.  FRISK_E_STATE without a finalised profile, FRISK_E_ARG for a push into a full panel
 *   (FRISK_PANEL_MAX slots); either leaves the panel as it was.  Memory: tiles of FRISK_PANEL_TILE slots, 64 bytes x 4^kmax each
 *   (4 MB at K = 8, 1 GB at K = 12), allocated as the panel grows.
 * frisk_panel_reset empties the panel and frees its memory (frisk_destroy does too); frisk_panel_size = P, its profiles.
 * frisk_score_ranges_panel: status and kld hold P planes of n rows, plane p = [p*n, (p+1)*n).  Row r of plane p is bit for bit
 *   what frisk_score_ranges returns for that range when profile p is the context's finalised profile.  gc, pi, si, cri, nn and the
 *   status bits FRISK_ROW_KEPT and FRISK_ROW_NO_MAXMER do not depend on the profile: the value columns are written once, [n] each.
 *   FRISK_ROW_ZERO_WEIGHT can differ between planes (a max-mer without weight in one genome and not in another).  A range that the
 *   N rule drops has status 0 and NaN in every plane.
 *   flags: FRISK_SCAN_RIP and FRISK_RANGES_BIG as in frisk_score_ranges.  The same row and batch checks, with the same FRISK_E_ARG
 *   and nothing launched.  FRISK_E_STATE: an empty panel (the context's own profile is not needed).  n = 0 is FRISK_OK and touches
 *   no output.  A streamed batch is waited for.  The scan's plan and rows, the context's profile and frisk_score_ranges are left
 *   alone: a call of those before and after panel use returns the same bytes.
 * frisk_last_kernel_ms(ctx, 5) = the panel kernels' time of the last call. */
#define FRISK_PANEL_MAX  64      /* profiles a context's panel can hold */
#define FRISK_PANEL_TILE  8      /* profiles scored per walk of a region's table */
int     frisk_panel_reset(frisk_ctx* ctx);
int     frisk_panel_push(frisk_ctx* ctx, int32_t* slot);
int32_t frisk_panel_size(const frisk_ctx* ctx);
int     frisk_score_ranges_panel(frisk_ctx* ctx, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                 uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri,
                                 int64_t* nn);

/* ---- the same rows, and the k-mers that drive each row's KLD --------------------------------
 * "Why does this region score as it does?"  A row's KLD is the sum of the reference's summands (KLD, L465-470) over its present
 * max-mers, term_k = pw_k * (ln(pw_k / pg_k) / ln 2); frisk_explain_ranges scores the rows as frisk_score_ranges does and keeps
 * the top_n largest terms of each (csrc/explain_kernels.h: a range is counted once and scored twice).
 * status, kld, gc, pi, si, cri, nn: bit for bit what frisk_score_ranges writes for the same rows.
 * n_present[r]: the distinct max-mers of a kept row; 0 for a row the N rule drops.
 * code, count, pw, pg, term: n * top_n entries each, row-major; slot j of row r is rank j, rank 0 the largest term.  Terms are
 *   compared as numbers (-0.0 equals +0.0); among equal terms the smaller code comes first.  code: the max-mer in the digit order
 *   of the tables (A, T, G, C = 0..3, first base most significant); count: its occurrences in the range; pw, pg: the two
 *   normalised IVOM values the reference's KLD sums over; term: pw * (ln(pw / pg) / ln 2), in that order of operations.
 *   A slot is filled only when status[r] is exactly FRISK_ROW_KEPT and j < min(top_n, n_present[r]); every other slot holds
 *   code 0xFFFFFFFF, count 0 and NaN in pw, pg and term.  The terms of over-represented max-mers are positive, those of
 *   under-represented present ones negative: a row with n_present <= top_n lists them all, and they sum to its kld.
 *   The selection is a function of the row's set of (term, code) pairs alone: a row's bits depend on the range and the profile,
 *   not on the other rows, their order, the form or the grid.
 * flags: FRISK_SCAN_RIP and FRISK_RANGES_BIG as in frisk_score_ranges.  The same row and batch checks, with the same FRISK_E_ARG
 * and nothing launched; FRISK_E_ARG too for top_n < 1, top_n > FRISK_EXPLAIN_MAX and a null required array (the six arrays here
 * included).  FRISK_E_STATE: no finalised profile.  n = 0 is FRISK_OK and touches no output.  A streamed batch is waited for.  The
 * scan's plan and rows, the panel and frisk_score_ranges are left alone.  Memory: 12 bytes per workgroup and entry of
 * min(longest range, 4^kmax), for the length of the call.
 * frisk_last_kernel_ms(ctx, 7) = the explain kernels' time of the last call. */
#define FRISK_EXPLAIN_MAX 64
int frisk_explain_ranges(frisk_ctx* ctx, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                         uint32_t flags, int32_t top_n,
                         uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri, int64_t* nn,
                         int32_t* n_present, uint32_t* code, uint32_t* count, double* pw, double* pg, double* term);

/* ---- a region's boundaries, to the base -----------------------------------------------------
 * "Where does this region start and end?"  Every region the scanner yields has boundaries on a window grid; frisk_refine_ranges
 * moves each boundary within +- flank bases to a likelihood-ratio change point (csrc/refine_kernels.h; frisk_amd/refine.py restates
 * it in numpy with the same integers).  Integer arithmetic only: a row's outputs are exactly reproducible.
 * Row r is (seq_index[r], a = start[r], b = stop[r]), 0-based half-open; F = flank, 1 <= F <= 65 536; the chain's order r = order
 * with kmin <= r + 1 <= kmax (the rule of frisk_seq_null); L = the scaffold's length.  Fe = min(F, (b - a) / 4) = flank_used[r].
 *   core    [a + Fe, b - Fe), counted as frisk_score_ranges counts a slice (no word past its ends, lowercase counts in words).
 *           status[r], nn[r] are the core's: nn as in frisk_score_ranges; FRISK_ROW_KEPT, FRISK_ROW_NO_MAXMER as there;
 *           FRISK_ROW_ZERO_WEIGHT for a max-mer present and kmin-1 <= S <= kmax-1 only (the genome's weights are not looked at).
 *           Fe = 0 (fewer than 4 bases: the core is the region) or a core the N rule drops (status 0): new_start = a, new_stop = b,
 *           both gains 0.
 *   models  one table of order r + 1 each; digits A, T, G, C = 0..3, first base most significant, word c has the context c >> 2.
 *           island: n_i(c) = the core's count of c; host: n_h(c) = the finalised profile's symmetric count of c; T(ctx) = the sum
 *           over the context's four words.  lp(n, T) = flog2(n + 1) - flog2(T + 4) (Laplace), qtab(c) = lp(n_i(c), T_i(c >> 2)) -
 *           lp(n_h(c), T_h(c >> 2)): int64 in units of 2^-32 bit.
 *   flog2   for an integer 1 <= x < 2^63: e = the index of its top bit, m = x << (63 - e) (Q1.63), f = 0; 32 times: p = m * m
 *           (128 bits), hi = p >> 64, f <<= 1; if hi >= 2^63: f |= 1, m = hi; else m = (hi << 1) | (low64(p) >> 63).  flog2(x) =
 *           (e << 32) + f, and 0 <= 2^32 log2 x - flog2(x) < 1 + 2^-20.
 *   q_j     at position j of the scaffold: qtab(the word of bases [j - r, j], upper-cased) when j - r >= 0 and none of its r + 1
 *           bases is invalid, else 0.  A word never crosses a scaffold's edge.
 *   start   G_s(t) = sum_{j = t}^{a + Fe - 1} q_j for t in [max(0, a - Fe), a + Fe]; new_start[r] = the LARGEST t that maximises it;
 *           gain_start[r] = G_s(new_start) - G_s(a) >= 0.
 *   stop    G_e(u) = sum_{j = b - Fe}^{u - 1} q_j for u in [b - Fe, min(L, b + Fe)]; new_stop[r] = the SMALLEST u that maximises it;
 *           gain_stop[r] = G_e(new_stop) - G_e(b) >= 0.
 * On a tie the shorter region wins (an N run across a boundary is left outside); new_start <= a + Fe < b - Fe <= new_stop.  Gains
 * are in units of 2^-32 bit.  A row's outputs depend on the row, the batch, the profile, F and r alone - not on the other rows,
 * their order, the form or the grid.
 * flags: FRISK_RANGES_BIG as in frisk_score_ranges; other bits are ignored.  The row and batch checks of frisk_score_ranges, with
 * the same FRISK_E_ARG and nothing launched; FRISK_E_ARG too for a flank or an order outside the above and for a null array.
 * FRISK_E_STATE: no finalised profile.  n = 0 is FRISK_OK and touches no output.  A streamed batch is waited for.  The scan's plan
 * and rows, the panel, frisk_score_ranges and frisk_explain_ranges are left alone.
 * frisk_last_kernel_ms(ctx, 8) = the refine kernels' time of the last call. */
int frisk_refine_ranges(frisk_ctx* ctx, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                        uint32_t flags, int32_t flank, int32_t order,
                        uint32_t* status, int64_t* nn, int64_t* new_start, int64_t* new_stop,
                        int64_t* gain_start, int64_t* gain_stop, int64_t* flank_used);

/* Test utility (kmax <= 6): the two distributions IvomBuild returns for each candidate window of [c0,c1) (L1481-1482, L369-457) -
 * window-side and genome-side interpolated probabilities of the window's present max-mers, each normalised to sum 1 -
 * as dense vectors of 4^kmax doubles per candidate (0 for absent max-mers; all 0 for windows the reference drops). */
int frisk_scan_ivom(frisk_ctx* ctx, int32_t w, int32_t inc, uint32_t flags, int64_t c0, int64_t c1, int64_t cap,
                    double* window_ivom, double* genome_ivom);

/* Diagnostics of the most recent frisk_scan (results never depend on them).  The default K = 8 kernel counts max-mers in
 * 4- or 8-bit counters and hands a window with a more frequent max-mer (low-complexity sequence) to the next wider form:
 * which = 0: counter width of the bulk launch (4 or 8; 16 = the narrow kernel was not used),
 *         1: windows handed from 4-bit to 8-bit counters,   2: windows handed on to 16-bit counters,
 *         3: row segments (2: the last sixteenth of a long scan ran on a second stream while the rows of the rest went to the host),
 *         4: 1 = the 4-bit bulk launch counted the max-mers of period <= 4 in its side table (FRISK_SCAN_SIDE4 / picked by the sample),
 *         5: 1 = the 4-bit bulk launch ran the kernel compiled for the lowest order 1 (K = 8, kmin = 1, no FRISK_SCAN_GENERIC). */
int64_t frisk_last_scan_stat(const frisk_ctx* ctx, int which);

/* The rows of the score table as text, exactly as the reference's scan loop writes them (L1487-1494): tab-separated
 * name, start, stop, windowKLD, GC[, PI, SI, CRI], one line per row, every value as Python 2's str() prints it (floats:
 * 12 significant digits, '.0' on integral values, nan / inf).  Host-side, multi-threaded; replaces a per-row Python loop
 * that costs tens of seconds at 3 M rows.  names: one per scaffold; kld_is_int0 (nullable): rows whose KLD is the int 0
 * (L465: no max-mer); pi/si/cri: all three or none.  Returns a malloc'd, NUL-terminated buffer (frisk_free) and its length. */
char* frisk_format_rows(int64_t n_rows, const char* const* names, const int32_t* seq_index, const int64_t* start,
                        const int64_t* stop, const uint8_t* kld_is_int0, const double* kld, const double* gc,
                        const double* pi, const double* si, const double* cri, int64_t* out_len);
void frisk_free(void* ptr);

/* Host-only: the 2-state, one-feature Gaussian HMM that segments the KLD track - what the reference asks of hmmlearn's
 * GaussianHMM(n_components=2, covariance_type="full") at L1539-1541 (fit on all non-NaN window scores stacked as one sequence)
 * and at L769 inside hmm2BED (Viterbi path per scaffold).  The model is the one frisk_amd/hmm.py documents (Baum-Welch with
 * hmmlearn's default priors, deterministic 2-means start, state 0 = the lower mean); this is its multi-threaded form for the
 * 3 M windows of a GRCh38-sized run.  frisk_hmm_fit: x[n] finite; n_iter / tol / min_covar / covars_prior as hmmlearn's
 * arguments (10, 1e-2, 1e-3, 1e-2); outputs means[2], covars[2], startprob[2], transmat[4] (row-major), the log-likelihood of
 * the last E step and the number of EM rounds run (nullable).  frisk_hmm_viterbi: n_seg sequences x[seg_off[s] .. seg_off[s+1])
 * decoded independently into states[] (0 / 1), one task per sequence. */
int frisk_hmm_fit(const double* x, int64_t n, int32_t n_iter, double tol, double min_covar, double covars_prior, double* means,
                  double* covars, double* startprob, double* transmat, double* loglik, int32_t* iters);
int frisk_hmm_viterbi(const double* x, const int64_t* seg_off, int32_t n_seg, const double* means, const double* covars,
                      const double* startprob, const double* transmat, int8_t* states);

/* Test utility: ONE E step of the given model over x[n], by the code a round of frisk_hmm_fit runs (csrc/hmm_host.h, e_step).
 * post_out (n x 2, nullable) receives the posteriors; stats_out[9] the sums over the windows of gamma_0, gamma_1, gamma_0 x,
 * gamma_1 x, xi_00, xi_01, xi_10, xi_11 and the log-likelihood.  FRISK_E_ARG for n < 1, a non-finite score or model value, a
 * variance <= 0, a probability outside [0, 1]. */
int frisk_hmm_estep(const double* x, int64_t n, const double* means, const double* covars, const double* startprob,
                    const double* transmat, double* post_out, double* stats_out);

/* The same model on `device` (csrc/hmm_kernels.h), without a context: host arrays in and out, FP64 throughout, bit-identical from
 * run to run (the sequence is cut into a number of pieces that depends on n alone, the sufficient statistics are added in a fixed
 * order, no floating-point atomics); the stop rule of the fit is evaluated in double on the host once per round.  Arguments and
 * results as frisk_hmm_fit / frisk_hmm_viterbi; the fitted numbers agree with the host form to rounding (a different exp / log
 * and reassociated sums), the Viterbi states are those of the host form wherever no decision is closer than rounding (ties to
 * the lower state).  FRISK_E_ARG on a bad argument (n < 1, non-finite scores - for the Viterbi form inside the decoded
 * range [seg_off[0], seg_off[n_seg]) -, a decreasing seg_off), checked before any device is touched; FRISK_E_HIP otherwise. */
int frisk_hmm_fit_gpu(int device, const double* x, int64_t n, int32_t n_iter, double tol, double min_covar, double covars_prior,
                      double* means, double* covars, double* startprob, double* transmat, double* loglik, int32_t* iters);
int frisk_hmm_viterbi_gpu(int device, const double* x, const int64_t* seg_off, int32_t n_seg, const double* means,
                          const double* covars, const double* startprob, const double* transmat, int8_t* states);

/* Test utility: frisk_hmm_estep on `device`, by the code a round of frisk_hmm_fit_gpu runs (csrc/hmm_kernels.h, e_step): the same
 * arguments and results with the device in front; the argument checks come before any device is touched. */
int frisk_hmm_estep_gpu(int device, const double* x, int64_t n, const double* means, const double* covars,
                        const double* startprob, const double* transmat, double* post_out, double* stats_out);

/* Projection and clustering of the anomalous windows' k-mer proportions (the reference's L1597-1697: sklearn PCA, DBSCAN and
 * KMeans), on `device`, without a context.  Inputs and outputs are host arrays (row-major); every result is bit-identical from
 * run to run (fixed-order reductions, no floating-point atomics).  Each returns FRISK_OK, FRISK_E_ARG on a bad argument (n < 1,
 * d > f, eps <= 0 or NaN, k < 1 or k > n, non-finite data, points of more than 64 dimensions for the two clusterings)
 * or FRISK_E_HIP.
 * frisk_proj_cov: mean_out[f] = column means of X[n][f]; cov_out[f][f] = (X - mean)T (X - mean) / (n - 1) (two-pass centring,
 *   FP64 matrix cores; n = 1 divides by 1).
 * frisk_proj_transform: Y_out[n][d] = (X - mean) V for V[f][d] (column q = component q).
 * frisk_dbscan: labels_out[n] of DBSCAN with Euclidean distance (neighbours: sqrt(sum of squares) <= eps, the point itself
 *   included; core: >= min_samples neighbours); clusters numbered 0, 1, ... in increasing order of their smallest core index,
 *   a border point in the first cluster that reaches it, noise -1 - sklearn's dbscan_inner labelling.
 * frisk_kmeans: Lloyd's algorithm from init_centers[k][d] until the labels stop changing, the squared centre shift is <= tol, or
 *   max_iter steps; then one more assignment to the final centres.  labels_out[n] (nearest centre, lowest index on a tie),
 *   centers_out[k][d], the inertia of that assignment and the steps run (both nullable).  Empty clusters follow sklearn's Lloyd
 *   step: unless every point sits on its centre, they take, in increasing id, the points farthest from their centres (descending
 *   distance, lowest index on a tie), each moved out of its own cluster; a cluster still empty is placed on the cluster of
 *   largest weight (its centre if that cluster's id is lower, its coordinate sum otherwise, as sklearn's _average_centers). */
int frisk_proj_cov(int device, const double* X, int64_t n, int64_t f, double* mean_out, double* cov_out);
int frisk_proj_transform(int device, const double* X, const double* mean, const double* V, int64_t n, int64_t f, int32_t d,
                         double* Y_out);
int frisk_dbscan(int device, const double* Y, int64_t n, int32_t d, double eps, int32_t min_samples, int32_t* labels_out);
int frisk_kmeans(int device, const double* Y, int64_t n, int32_t d, int32_t k, const double* init_centers, int32_t max_iter,
                 double tol, int32_t* labels_out, double* centers_out, double* inertia_out, int32_t* n_iter_out);

/* Exact t-SNE of the reference's --runProjection PY-TSNE (frisk/tsne.py: x2p, then 1000 iterations of gradient descent with
 * momentum, gains and early exaggeration), FP64 on `device`.  The handle keeps X, the affinities and the optimiser state (Y, iY,
 * gains) on the device between calls, so a caller can step the optimiser; every result is bit-identical from run to run.
 * frisk_tsne_create: X[n][f] (the input after the caller's PCA step), perplexity, dims output columns, Y0[n][dims] the start;
 *   iY = 0 and gains = 1.  FRISK_E_ARG, with nothing allocated, unless 2 <= n <= 50 000, 1 <= f <= 64, 1 <= dims <= 64,
 *   perplexity > 0 and X, Y0 and perplexity finite.  Device memory: 8 n^2 bytes for the affinities plus O(n (f + dims)).
 * frisk_tsne_affinities: computes the affinities once (later calls only copy): squared distances by direct differences; per row
 *   the reference's bisection on beta from 1 (target entropy log(perplexity), tolerance 1e-5, at most 50 tries); P + PT
 *   normalised by its total; q = max(that, 1e-12 / 4), so that the reference's P is 4 q for iterations 0 .. 100 and q after.
 *   Outputs (each nullable): beta_out[n], tries_out[n], q_out[n][n].  FRISK_E_ARG when a row's sum of exp(-D beta) is 0 or not
 *   finite (the reference's row would be NaN).
 * frisk_tsne_run: iterations t = iter_begin .. iter_end - 1 (0 <= iter_begin <= iter_end <= 1000) on one stream, without a host
 *   sync inside; momentum (0.5 for t < 20, then 0.8) and exaggeration (t <= 100) follow from t, so run(0, 1000) equals run(0, 400)
 *   then run(400, 1000) bit for bit.  cost_out (nullable): the reference's logged cost sum P log(P / Q) of every t with
 *   (t + 1) % 10 == 0, in order.  Computes the affinities first if frisk_tsne_affinities has not.
 * frisk_tsne_get / frisk_tsne_set: the state Y, iY, gains (each [n][dims], each nullable); set rejects non-finite values. */
typedef struct frisk_tsne frisk_tsne;
int  frisk_tsne_create(int device, const double* X, int64_t n, int32_t f, double perplexity, int32_t dims, const double* Y0,
                       frisk_tsne** out);
int  frisk_tsne_affinities(frisk_tsne* h, double* beta_out, int32_t* tries_out, double* q_out);
int  frisk_tsne_run(frisk_tsne* h, int32_t iter_begin, int32_t iter_end, double* cost_out);
int  frisk_tsne_get(frisk_tsne* h, double* Y, double* iY, double* gains);
int  frisk_tsne_set(frisk_tsne* h, const double* Y, const double* iY, const double* gains);
void frisk_tsne_destroy(frisk_tsne* h);

/* Metric MDS of the reference's --runProjection MDS (sklearn.manifold.MDS(metric=True, dissimilarity='euclidean'): the SMACOF
 * algorithm of sklearn's _smacof_single), FP64 on `device`.  The handle keeps the n x n dissimilarities on the device, so a caller
 * can run several starts, or step the algorithm, against one D; every result is bit-identical from run to run.
 * frisk_mds_create: X[n][f] (the raw k-mer proportions), dims output columns; computes D_ij = sqrt(sum_k (x_ik - x_jk)^2) by
 *   direct differences (exactly symmetric, diagonal exactly 0).  FRISK_E_ARG, with nothing allocated, unless 2 <= n <= 50 000,
 *   f >= 1, 1 <= dims <= 64 and X finite.  Device memory: 8 n^2 bytes for D plus O(n (f + dims)).
 * frisk_mds_dissimilarities: D_out[n][n] = D.
 * frisk_mds_run: SMACOF from Y0[n][dims]: each step sets configuration distances that are exactly 0 to 1e-5, X <- (1 / n) B X
 *   with B = -D / dist plus its row sums on the diagonal (computed as sum_j D_ij / dist_ij (x_i - x_j)), then the raw stress
 *   sum over all i, j of (dist_ij - D_ij)^2 / 2 of the new X; from the second step on it stops when
 *   (previous stress - stress) / (sum over all i, j of dist_ij^2 / 2) < eps, evaluated on the host in double, or after max_iter
 *   steps.  Y_out[n][dims] the final X, stress_out its raw stress, n_iter_out the steps run (both nullable); stress_trace_out
 *   (nullable, room for max_iter values) the stress after each step.  With eps = 0 the run stops early only if the stress
 *   rises, so run(Y_t, 1, 0) is one step.  FRISK_E_ARG for non-finite Y0, max_iter < 1, or eps < 0 or not finite. */
typedef struct frisk_mds frisk_mds;
int  frisk_mds_create(int device, const double* X, int64_t n, int64_t f, int32_t dims, frisk_mds** out);
int  frisk_mds_dissimilarities(frisk_mds* h, double* D_out);
int  frisk_mds_run(frisk_mds* h, const double* Y0, int32_t max_iter, double eps, double* Y_out, double* stress_out,
                   int32_t* n_iter_out, double* stress_trace_out);
void frisk_mds_destroy(frisk_mds* h);

/* Incremental PCA of the reference's --runProjection IncrementalPCA (sklearn.decomposition.IncrementalPCA(n_components=d,
 * whiten=False, batch_size=None)), FP64 on `device`.  The handle keeps the fit on the device between batches: the rows seen, the
 * column mean and variance (sklearn's _incremental_mean_and_var, operation for operation), the singular values S[d] and the
 * components Vt[d][f].  One batch is two calls, with the eigendecomposition of the Gram matrix between them left to the caller:
 * frisk_ipca_create: f features, d components.  FRISK_E_ARG unless f >= 1 and 1 <= d <= f.
 * frisk_ipca_gram: X[b][f], one batch.  Computes the batch's mean / variance update and G_out[f][f] = AT A (exactly symmetric),
 *   where A is the batch minus the new mean (first batch) or the stack of the d rows S_i Vt_i, the batch minus its own mean
 *   and the row sqrt(seen / (seen + b) * b) (old mean - batch mean).  The eigenvectors of G are the right singular vectors of A,
 *   its eigenvalues their squared singular values.  The fit itself does not change.  FRISK_E_ARG for b < 1, a first batch with
 *   b < d, or a non-finite X.
 * frisk_ipca_commit: S[d], Vt[d][f] of the batch last given to frisk_ipca_gram become the fit, with that batch's mean, variance
 *   and row count.  FRISK_E_STATE without such a batch.
 * frisk_ipca_get: n_seen, mean[f], var[f], S[d], Vt[d][f] of the fit (each nullable; FRISK_E_STATE for an array before the
 *   first commit).  frisk_ipca_set replaces the fit (n_seen = 0: back to the unfitted state, the arrays are not read) and
 *   drops a batch not yet committed.
 * frisk_ipca_transform: Y_out[n][d] = (X - mean) V for any n >= 1, rows fed to the device in pieces; FRISK_E_STATE before the
 *   first commit.
 * frisk_ipca_last_ms: device time of the last frisk_ipca_gram in ms: which = 0 upload, 1 statistics + stack, 2 Gram; else -1.
 * Every result is bit-identical from run to run. */
typedef struct frisk_ipca frisk_ipca;
int  frisk_ipca_create(int device, int64_t f, int32_t d, frisk_ipca** out);
int  frisk_ipca_gram(frisk_ipca* h, const double* X, int64_t b, double* G_out);
int  frisk_ipca_commit(frisk_ipca* h, const double* S, const double* Vt);
int  frisk_ipca_get(frisk_ipca* h, int64_t* n_seen, double* mean, double* var, double* S, double* Vt);
int  frisk_ipca_set(frisk_ipca* h, int64_t n_seen, const double* mean, const double* var, const double* S, const double* Vt);
int  frisk_ipca_transform(frisk_ipca* h, const double* X, int64_t n, double* Y_out);
double frisk_ipca_last_ms(const frisk_ipca* h, int which);
void frisk_ipca_destroy(frisk_ipca* h);

/* NMF of the reference's --runProjection NMF (sklearn.decomposition.NMF(n_components=d, init=None, solver='cd', shuffle=False):
 * the coordinate descent of _fit_coordinate_descent / _update_cdnmf_fast with the identity permutation, no regularisation), FP64
 * on `device`.  The handle keeps X[n][f], W[n][d] and H[d][f] on the device; the caller drives the iterations and evaluates
 * sklearn's stop rule in double from the violation each step returns.  The two products are public because the initialisation
 * (sklearn's randomized range finder) needs them on X as well.
 * frisk_nmf_create: X[n][f], d components; W and H start as zeros.  FRISK_E_ARG, with nothing allocated, unless n >= 1, f >= 1,
 *   1 <= d <= 16 and every entry of X is finite and >= 0.  Device memory: 8 n f bytes for X plus O((n + f) * 26) and the split
 *   partials of frisk_nmf_xtq (at most 256 * f * 26 doubles).
 * frisk_nmf_xq: Y_out[n][p] = X Q for Q[f][p];  frisk_nmf_xtq: Z_out[f][p] = XT Q for Q[n][p].  FRISK_E_ARG unless 1 <= p <= 26
 *   and Q is finite.
 * frisk_nmf_step: one iteration.  The W sweep against HHt = H HT and X HT: for each row s and t = 0 .. d - 1 in order,
 *   g = -XHt[s][t] + sum_r HHt[t][r] W[s][r] (r in order), pg = W[s][t] == 0 ? min(0, g) : g, and W[s][t] = max(W[s][t] -
 *   g / HHt[t][t], 0) where HHt[t][t] != 0; then, with update_H != 0, the same sweep of HT against WT W and XT W.  *violation =
 *   the sum of |pg| of the W sweep plus that of the H sweep.  W_inout[n][d] and H_inout[d][f] are nullable: a given array
 *   replaces the state on the device before the step and receives it after; with null the state stays on the device.
 * frisk_nmf_get / frisk_nmf_set: W[n][d], H[d][f] (each nullable).  FRISK_E_ARG for a non-finite entry.
 * frisk_nmf_transform_prepare: computes H HT and X HT of the current H once; steps with update_H == 0 reuse them until H is set
 *   or updated (a step with update_H == 0 leaves them valid for the next one in the same way).  The results do not change.
 * frisk_nmf_last_ms: device time in ms of the last call: which = 0 X Q (frisk_nmf_xq, or X HT within a step), 1 XT Q
 *   (frisk_nmf_xtq, or XT W within a step), 2 the whole of the last step; else -1.
 * Every result is bit-identical from run to run. */
typedef struct frisk_nmf frisk_nmf;
int  frisk_nmf_create(int device, const double* X, int64_t n, int64_t f, int32_t d, frisk_nmf** out);
int  frisk_nmf_xq(frisk_nmf* h, const double* Q, int32_t p, double* Y_out);
int  frisk_nmf_xtq(frisk_nmf* h, const double* Q, int32_t p, double* Z_out);
int  frisk_nmf_step(frisk_nmf* h, double* W_inout, double* H_inout, int32_t update_H, double* violation);
int  frisk_nmf_get(frisk_nmf* h, double* W, double* H);
int  frisk_nmf_set(frisk_nmf* h, const double* W, const double* H);
int  frisk_nmf_transform_prepare(frisk_nmf* h);
double frisk_nmf_last_ms(const frisk_nmf* h, int which);
void frisk_nmf_destroy(frisk_nmf* h);

/* Spectral clustering of the reference's --cluster SPECTRAL (sklearn.cluster.SpectralClustering(affinity='rbf', gamma,
 * assign_labels='kmeans')): the dense n x n part, FP64 on `device`.  The handle keeps ONE n x n buffer on the device: the
 * affinities A0_ij = exp(-gamma sum_c (y_ic - y_jc)^2) (direct differences, c in order; the diagonal exactly 0, A0 exactly
 * symmetric), normalised in place as scipy.sparse.csgraph.laplacian(normed=True) does: w_j = sum_i A0_ij (the rows in fixed
 * ranges, the ranges in order), w == 0 replaced by 1, dd = sqrt(w), M_ij = (A0_ij / dd_j) / dd_i.  scipy's entry (j, i) divides
 * in the other order and can differ in the last two roundings; each entry here is the mean of the two, so M is exactly symmetric and
 * within 1 ulp of scipy's entry on either side.  The caller drives the eigen-iteration with products against M (block subspace
 * iteration with Rayleigh-Ritz: frisk_amd.projection.spectral_embedding); the host parts are at most 26 columns wide.
 * frisk_spectral_create: Y[n][d]; computes A0, dd and M.  FRISK_E_ARG, with nothing allocated, unless 2 <= n <= 50 000,
 *   1 <= d <= 64, gamma is finite and > 0 and every entry of Y is finite.  Device memory: 8 n^2 bytes plus O(n * (256 + 52 + d)).
 * frisk_spectral_affinity: A0_out[n][n], before normalisation: recomputed into the buffer on request (the same bits), copied out,
 *   and the buffer normalised again from the kept dd (the same M).
 * frisk_spectral_degrees: dd_out[n], and *n_isolated = the number of points whose w was 0 (every affinity underflowed).
 * frisk_spectral_matrix: M_out[n][n].
 * frisk_spectral_mq: Z_out[n][p] = M Q for Q[n][p].  FRISK_E_ARG unless 1 <= p <= 26 and Q is finite.
 * frisk_spectral_last_ms: device time in ms of the last affinity computation (which = 0), degrees + normalisation at create (1),
 *   and the last product (2); else -1.
 * Every entry point returns FRISK_E_ARG for a null pointer.  Every result is bit-identical from run to run. */
typedef struct frisk_spectral frisk_spectral;
int  frisk_spectral_create(int device, const double* Y, int64_t n, int32_t d, double gamma, frisk_spectral** out);
int  frisk_spectral_affinity(frisk_spectral* h, double* A0_out);
int  frisk_spectral_degrees(frisk_spectral* h, double* dd_out, int64_t* n_isolated);
int  frisk_spectral_matrix(frisk_spectral* h, double* M_out);
int  frisk_spectral_mq(frisk_spectral* h, const double* Q, int32_t p, double* Z_out);
double frisk_spectral_last_ms(const frisk_spectral* h, int which);
void frisk_spectral_destroy(frisk_spectral* h);

/* sklearn 1.7's TSNE of the reference's --runProjection SKL-TSNE (TSNE(early_exaggeration=4, learning_rate=1000, max_iter=1000,
 * n_iter_without_progress=30, min_grad_norm=1e-7, angle=0.5), method 0 = 'exact', 1 = 'barnes_hut').  The handle keeps X, the
 * affinities and the float32 state (Y, update, gains) on `device`; the caller drives the descent 50 iterations at a time and applies
 * sklearn's stop rule (frisk_amd.projection.skl_tsne_descent).  Squared distances by direct differences in FP64, rounded to float32;
 * _binary_search_perplexity as written (beta from 1, at most 100 steps, tolerance (float)1e-5).  The gradient, the normaliser and the
 * error are accumulated in FP64, the gradient rounded to float32 once, the update with gains done in float32 in sklearn's order.
 * barnes_hut keeps the k = min(n - 1, (int)(3 perplexity + 1)) nearest neighbours of each row and sums the repulsive term over ALL
 * pairs: sklearn's own result in the limit angle -> 0, not its angle = 0.5 tree approximation.
 * frisk_skltsne_create: X[n][f], any f >= 1.  FRISK_E_ARG, with nothing allocated, unless 2 <= n <= 50 000, 0 < perplexity < n,
 *   1 <= dims <= 64 (exact) or 3 (barnes_hut) and X is finite.  Y starts at 0, update at 0, gains at 1.  Device memory: exact
 *   8 n^2 bytes, barnes_hut 12 n k bytes, plus 8 n f and O(n dims).
 * frisk_skltsne_affinities: computes the affinities once (later calls only copy).  beta_out[n]: the beta each row's probabilities
 *   were computed with; steps_out[n]: the bisection step that met the tolerance (0 .. 99), 100 when none did.  Both nullable.
 * frisk_skltsne_p_dense (exact, after affinities): P_out[n][n] = max((C + CT) / max(sum, eps), eps), 0 on the diagonal.
 * frisk_skltsne_neighbours (barnes_hut, after affinities): indices_out[n][k], each row's neighbours in ascending column order (the
 *   k smallest float32 distances, ties to the lower column), and cond_out[n][k], their p_j|i.  Both nullable.
 * frisk_skltsne_set_p (barnes_hut): the symmetrised, normalised joint probabilities as CSR (indptr[n + 1], indices[nnz] in [0, n),
 *   float32 values[nnz]), which the caller builds from the conditionals as sklearn's _joint_probabilities_nn does.
 * frisk_skltsne_get / frisk_skltsne_set: the state Y, update, gains (each float[n][dims], each nullable); set rejects non-finite values.
 * frisk_skltsne_run: iterations iter_begin .. iter_end - 1 (0 <= iter_begin < iter_end <= 1000) with P multiplied by `exaggeration`,
 *   no host synchronisation inside.  *error = the KL divergence and *grad_norm = |grad * gains|_2 of the last of them.
 *   FRISK_E_STATE for barnes_hut before frisk_skltsne_set_p; exact computes its affinities first if need be.
 * frisk_skltsne_last_ms: device time in ms of the affinities (which = 0) and of the last run (1); else -1.
 * Every entry point returns FRISK_E_ARG for a null handle.  Every result is bit-identical from run to run. */
typedef struct frisk_skltsne frisk_skltsne;
int  frisk_skltsne_create(int device, const double* X, int64_t n, int64_t f, double perplexity, int32_t dims, int32_t method,
                          frisk_skltsne** out);
int  frisk_skltsne_affinities(frisk_skltsne* h, double* beta_out, int32_t* steps_out);
int  frisk_skltsne_p_dense(frisk_skltsne* h, double* P_out);
int  frisk_skltsne_neighbours(frisk_skltsne* h, int32_t* indices_out, double* cond_out);
int  frisk_skltsne_set_p(frisk_skltsne* h, const int64_t* indptr, const int32_t* indices, const float* values, int64_t nnz);
int  frisk_skltsne_get(frisk_skltsne* h, float* Y, float* update, float* gains);
int  frisk_skltsne_set(frisk_skltsne* h, const float* Y, const float* update, const float* gains);
int  frisk_skltsne_run(frisk_skltsne* h, int32_t iter_begin, int32_t iter_end, double momentum, double exaggeration, double* error,
                       double* grad_norm);
double frisk_skltsne_last_ms(const frisk_skltsne* h, int which);
void frisk_skltsne_destroy(frisk_skltsne* h);

/* Page-locked host memory for result buffers: D2H copies into it are asynchronous and run at PCIe rate
 * (pageable buffers work too, at a fraction of it).  Free with frisk_host_free before frisk_destroy. */
void* frisk_host_alloc(frisk_ctx* ctx, int64_t bytes);
void  frisk_host_free(frisk_ctx* ctx, void* ptr);

/* Timing of the most recent launches on the context's stream, measured with HIP events:
 * which = 0 scan kernel, 1 profile_add kernel, 2 pack kernel, 3 frisk_window_vectors' kernels, 4 frisk_score_ranges' kernels,
 * 5 frisk_score_ranges_panel's kernels, 6 frisk_seq_null's generator kernels, 7 frisk_explain_ranges' kernels,
 * 8 frisk_refine_ranges' kernels (the host table, both forms).  Returns milliseconds, <0 if none. */
double frisk_last_kernel_ms(const frisk_ctx* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif /* FRISK_HIP_H */
