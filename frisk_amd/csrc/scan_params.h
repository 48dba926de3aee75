// scan_params.h - what the host side of a scan and its kernels share: the kernel arguments, the row status bits, the LDS carve-up of
// the 16-bit form and the sizes the host reads.  No kernel lives here: frisk_abi.hip includes this header, and only
// scan_launch.hip / scan8_launch.hip include the kernels (a non-template __global__ function may be compiled into one unit only).
#pragma once
#include "frisk_device.h"

#define FRISK_T8_BYTES 131072

struct ScanParams {
    const uint32_t* codes;
    const uint32_t* inv;
    const uint32_t* low;
    const ScafDesc* descs;
    const double* ig;         // genome-side IVOM, 4^kmax entries (NaN = zero weight)
    const double* log_tab;    // FRISK_LOGTAB_N pairs {1/c_i, ln c_i}: range reduction of log_tab_pos()
    const double* log_tab64;  // the same with 64 bins (scan8_kernel.h, where LDS is short)
    const double* log_tab32;  // ... and with 32
    int32_t n_desc;
    int32_t kmin, kmax;
    int32_t w, inc;
    uint32_t flags;           // FRISK_SCAN_*
    int64_t c0, c1;           // candidate range
    int32_t chunk;            // consecutive candidates handed to a workgroup at a time
    int32_t orphan_cap;       // capacity of the orphan list (entries)
    int32_t lv;               // shared_level(), or 0 when the prefix tables do not fit beside a long window's orphan list
    int32_t nprof;            // profile length (debug dump stride)
    // outputs, indexed by (candidate - c0)
    int32_t* seq_index;
    int64_t* start;
    int64_t* stop;
    uint32_t* status;
    double* kld;              // scan_kernel leaves T = sum Iw ln(Iw/Ig) here, finish_rows_kernel turns it into the KLD
    double* gc;               // scan_kernel leaves {S << 32 | G+C} here, finish_rows_kernel the fraction
    double* sw;               // raw sums of the row: sum Iw ...
    double* sg;               // ... and sum Ig (NaN: a max-mer without genome weight)
    double* pi;
    double* si;
    double* cri;
    uint32_t* dbg_counts;
    int64_t* dbg_meta;
    double* dbg_ivom;             // debug, kmax <= 6: row x 2 x 4^kmax - un-normalised window-side and genome-side IVOM per max-mer
    unsigned long long* unused_stamps;  // always nullptr: kept so that the kernel-argument offsets of the fields below stay put
    // scan8_kernel.h (narrow order-8 counters): windows whose counters wrap are handed to the next wider form through
    // device-side lists of candidate indices
    const double* rc_tab;         // 1/c for c = 0..255 (entry 0 = 0): the weight of one of the c positions that share a max-mer
    const int64_t* in_list;       // != nullptr: take the candidates from in_list[0 .. *in_count) instead of [c0, c1)
    const unsigned int* in_count;
    int64_t* out_list;            // scan8_kernel appends the windows it could not hold ...
    unsigned int* out_count;      // ... and counts them
    int32_t sel_mode, sel_mod;    // scan8_kernel, range mode: 0 all chunks, 1 every sel_mod-th chunk, 2 all the others
    unsigned int* queue;          // scan8_kernel: != nullptr: chunks are dealt by these counters (zero at launch) instead of by block index:
    int32_t queue_n;              // ... queue_n (1 or 8) of them, one per XCD, each over a contiguous share of the chunks
    double* ig_ring;              // scan8_kernel: per-workgroup ring of genome-side values by window position (see scan8_kernel.h), or nullptr
    const unsigned int* verdict;  // scan8_kernel: != nullptr: this launch runs only if *verdict == my_form (the adaptive width's sample decides on the
    unsigned int my_form;         // ... device which of the bulk forms - 1 plain 4-bit, 2 4-bit + side table, 3 8-bit - scores the rest; the others return at once)
    int32_t slide_pp;             // scan8_kernel: > 0: inside a chunk the order-K table slides from window to window, this many positions of
                                  // the leaving and of the entering range per thread (= ceil(inc / threads)); 0: every window counted afresh
};

// The counter block of the narrow-counter path (frisk_ctx::d_ovf_count; zero when a scan's launches start): SCAN_CNT_TOTAL unsigned
// ints, SCAN_CNT_SEGMENT of them per row segment.  Entries of a segment:
enum ScanCounter {
    SCAN_CNT_LIST1 = 0,             // length of list 1 (windows that wrapped a 4-bit counter) ...
    SCAN_CNT_LIST2 = 1,             // ... and of list 2 (8-bit): ScanParams::in_count / out_count of the launches that walk / fill them
    SCAN_CNT_SAMPLE_WOULD = 2,      // the sample: windows it scored that a plain 4-bit counter would have handed on ...
    SCAN_CNT_SAMPLE_SCORED = 3,     // ... and windows it scored (both relative to the sample's out_count, which is the block's base)
    SCAN_CNT_BULK_QUEUES = 8,       // [8, 16): the bulk launch's chunk queues, SCAN_CNT_BULK_QUEUE_N of them, one per XCD
    SCAN_CNT_BULK_QUEUE_N = 8,
    SCAN_CNT_QUEUE8 = 16,           // the chunk queue of the 8-bit launch over list 1
    SCAN_CNT_SEGMENT = 32,          // stride from one row segment's counters to the next
    SCAN_CNT_TOTAL = 64             // the block: two segments
};

#define ROW_KEPT 1u
#define ROW_ZERO_WEIGHT 2u
#define ROW_JUMPBACK 4u
#define ROW_NO_MAXMER 8u

// LDS carve-up (dynamic, all offsets multiples of 16 bytes)
struct LdsLayout {
    uint32_t t8;        // byte offset of the order-8 table (K8 only)
    uint32_t small;     // byte offset of the small tables (orders kmin..ks), u16 bins
    uint32_t small_bytes;
    uint32_t orphans;   // u16 list
    uint32_t pre_i;     // f64[4^lv]: sum_{x<=lv} c_x^2 4^x/D_x of the lv-mer prefix
    uint32_t pre_w;     // u32[4^lv]: running weight sum after order lv
    uint32_t rtab;      // f64[16]: 4^x / ((S-(x-1))*2) per order x (window constants)
    uint32_t logtab;    // f64[2*FRISK_LOGTAB_N]: {1/c_i, ln c_i}, written once per workgroup
    uint32_t misc;      // 2 x 16 u32 counters (double-buffered by window parity) + reduction scratch
    uint32_t t8_bytes;  // 128 KiB at K = 8
    uint32_t total;
};

// order at which the recursion is shared between max-mers (0 = not shared)
__host__ __device__ inline int shared_level(int kmin, int kmax) { return (kmin <= 5 && kmax >= 6) ? 5 : 0; }

#define FRISK_MISC_SLOTS 16
#define FRISK_LOGTAB_N 128
#define FRISK_MISC_BYTES (2 * FRISK_MISC_SLOTS * 4 + 16 * 6 * 8)       // counters x2, scratch (16 waves x 3 x 128 bit)

__host__ __device__ inline LdsLayout make_layout(int kmin, int kmax, int orphan_cap, int lv) {
    LdsLayout L;
    const bool k8 = (kmax == 8);
    const int ks = k8 ? 6 : kmax;
    uint32_t o = 0;
    L.t8 = o;
    L.t8_bytes = k8 ? FRISK_T8_BYTES : 0;
    o += L.t8_bytes;
    L.small = o;
    int64_t bins = (ks >= kmin) ? table_offset(kmin, ks + 1) : 0;
    L.small_bytes = uint32_t((bins * 2 + 15) / 16 * 16);
    o += L.small_bytes;
    L.orphans = o;
    o += uint32_t((k8 ? orphan_cap : 0) * 2 + 15) / 16 * 16;
    L.pre_i = o;
    if (lv) o += (1u << (2 * lv)) * 8;
    L.pre_w = o;
    if (lv) o += (1u << (2 * lv)) * 4;
    L.rtab = o;
    o += 16 * 8;
    L.logtab = o;
    o += FRISK_LOGTAB_N * 16;
    L.misc = o;
    o += FRISK_MISC_BYTES;
    L.total = (o + 15) / 16 * 16;
    return L;
}

#define FRISK8_RING_PAD 16          // scan8_kernel.h: doubles behind every workgroup's slice of the ring, touched by nobody (the idle lanes of FRISK8_DEAL's
                                    // parking waves stored there, at c34d7fb); part of the slice stride
