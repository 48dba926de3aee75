// scan_schedule.h - the launch schedule of one frisk_scan as a plain value: every decision between the call's arguments and its
// launches (path, chunk length, static deal or counters, sliding, ring slices, the sample and its stride, bulk width and side
// table, the kernel form of every launch - scan_forms.h -, where the tail segment is cut, the packed row block), computed by a pure
// function.  No HIP here: frisk_abi.hip fills a ScanShape from the context and walks the ScanSchedule, handing each launch the form
// named here; tools/exp/san_host.cpp, scan_dispatch_host.cpp and scan_forms_host.cpp compute and check schedules on a CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/frisk_hip.h"      // FRISK_SCAN_*, FRISK_E_* (found without an include path of its own)
#include "scan_forms.h"             // Scan8Form, Scan16Form, FRISK_K7_WPS

#define FRISK_SIDE_SHARE 0.06       // 4-bit bulk takes the side-table form when the plain form would hand on more than this share of the sample
#define FRISK_K8_WIDTH 0            // order-8 counters of the default K = 8 path (scan8_kernel.h): 0 = adaptive 4/8 bits, 4, 8, 16 = off

// everything the decisions read
struct ScanShape {
    int32_t kmin, kmax, num_cu;
    int64_t n;                      // candidates of this call (c1 - c0), >= 1
    int32_t w, inc;
    uint32_t flags;                 // FRISK_SCAN_*
    int64_t plan_maxwin;            // the longest window of the plan (a rescued small scaffold may exceed w)
    bool debug, want_ivom, rip;
    // the resident batch's hint: the counter width the last sampled scan of the batch chose (0: none yet), and whether it was
    // taken with this call's w and inc
    int32_t width_hint, hint_side;
    bool hint_matches;
    // LDS of scan_kernel.h's workgroup - make_layout(kmin, kmax, scan_orphan_cap(plan_maxwin), lv).total - with the shared prefix
    // level lv_shared (= shared_level(kmin, kmax)) and with level 0
    int32_t lv_shared;
    uint32_t lds_shared, lds_level0;
    // tuning knobs of experiment builds (-DFRISK_TUNE), read from the environment by the caller; the product library sets none
    bool has_scan_chunk; int64_t scan_chunk;    // FRISK_SCAN_CHUNK
    bool has_k8_bits; int k8_bits;              // FRISK_K8_BITS
    bool one_wg;                                // FRISK_ONE_WG: never two workgroups per CU
    bool no_slide, no_deal, one_segment, tail_any;      // FRISK_NO_SLIDE, FRISK_NO_DEAL, FRISK_ONE_SEGMENT, FRISK_TAIL_ANY
};

// short scans: the row columns as consecutive pieces of one block - [start | stop | kld | gc | pi si cri | seq_index | status] - so
// that one copy brings them to the host.  Offsets in 8-byte words from the block's base.
struct RowBlock {
    size_t start, stop, kld, gc, pi, si, cri, seq_index, status, words;
};
inline RowBlock row_block(int64_t n, bool rip) {
    const size_t Np = (size_t(n) + 1) / 2 * 2;                  // (the two 4-byte columns end on a multiple of 8 bytes)
    RowBlock b;
    b.start = 0; b.stop = Np; b.kld = 2 * Np; b.gc = 3 * Np;
    b.pi = 4 * Np; b.si = 5 * Np; b.cri = 6 * Np;               // (with rip only)
    b.seq_index = (4 + (rip ? 3 : 0)) * Np;
    b.status = b.seq_index + Np / 2;
    b.words = b.seq_index + Np;
    return b;
}

enum ScanPath {
    SCAN_PATH_BIG,          // scan_big_kernel.h: windows beyond the 16-bit LDS counters, and every window at K > 8
    SCAN_PATH_NARROW,       // scan8_kernel.h: narrow order-K counters, overflowing windows handed to the wider forms
    SCAN_PATH_TWO_WG,       // scan_kernel.h, K <= 7: two independent 256-thread workgroups per CU
    SCAN_PATH_16BIT         // scan_kernel.h by window class
};

struct ScanSchedule {
    const char* error;      // != nullptr: the call is refused with this text and error_code, nothing below holds
    int error_code;
    ScanPath path;
    int32_t lv;             // ScanParams::lv
    uint32_t lds_total;     // dynamic LDS of scan_kernel.h's launches
    int grid;               // workgroups of scan_kernel.h's launch over the whole range
    int big_grid;           // ... of scan_big_kernel's (one per CU)
    int32_t chunk;          // ScanParams::chunk of that launch
    int its;                // scan_kernel.h's window class: positions per thread unrolled 4 / 10 / 16 times, 0 = runtime loops (1024 threads);
                            // on the two-workgroup path 8 / 20
    int32_t orphan_cap;
    // the narrow-counter path
    bool narrow8, small_w, can_slide, short_scan, dealt, sample, side;
    bool kmin1_form;        // the 4-bit bulk launches take scan8_kernel's instantiations with the lowest order compiled in (SCAN8_ROLE_KMIN1)
    int64_t chunk8;         // consecutive windows per chunk
    int32_t slide_pp;       // ScanParams::slide_pp
    int64_t ring_slices;    // workgroup slices of the genome-value ring, 0 = no ring
    int64_t nchunks;
    int32_t sel_mod;        // the sample's stride in chunks
    int64_t nsample;        // chunks of the sample
    int bulk;               // counter width of the bulk launch (16 off the narrow path); with `sample`: what the launch shapes assume until
                            // the device's verdict is read back
    int sel_mode;           // ScanParams::sel_mode of the bulk launch
    int64_t cut;            // rows [0, cut) on the context's stream, [cut, n) on the tail stream; == n: one segment
    int segments;
    bool packed_rows;
    RowBlock block;         // (with packed_rows)
    // The kernel form of every launch (scan_forms.h), derived from the decisions above.  form16: scan_kernel.h's launch - the whole
    // range off the narrow path, list 2 on it.  The narrow path: the sample, the bulk launch - or, with `sample`, the three that wait
    // for the device's verdict: form_verdict[v - 1] runs where the verdict is v (1 plain 4-bit, 2 4-bit + side table, 3 8-bit) -
    // and the 8-bit launch over list 1.  A launch that the schedule does not make has no form.
    Scan16Form form16;
    Scan8Form form_sample, form_bulk, form_verdict[3], form_handover;
};

inline int32_t scan_orphan_cap(int64_t plan_maxwin) { return int32_t(plan_maxwin / 8 + 2); }

inline ScanSchedule plan_scan_schedule(const ScanShape& s) {
    ScanSchedule S = ScanSchedule();
    const int64_t n = s.n;
    const bool debug = s.debug;
    S.packed_rows = n < (int64_t(1) << 17);
    if (S.packed_rows) S.block = row_block(n, s.rip);
    S.orphan_cap = scan_orphan_cap(s.plan_maxwin);
    S.sel_mod = 16; S.bulk = 16; S.cut = n; S.segments = 1;

    const bool k8 = (s.kmax == 8);
    // LDS budget: 160 KB per workgroup.  Long windows at K = 8 need a long orphan list; the shared prefix tables
    // (12 KB, an optimisation only) make room for it.
    S.lv = s.lv_shared;
    S.lds_total = s.lds_shared;
    if (S.lds_total > 160 * 1024 && S.lv) { S.lv = 0; S.lds_total = s.lds_level0; }
    if (s.kmax <= 8 && s.plan_maxwin <= 65535 && S.lds_total > 160 * 1024) {
        S.error = "window too long for the 160 KB LDS of one workgroup";
        S.error_code = FRISK_E_ARG;
        return S;
    }
    const int wg_per_cu = std::max(1, std::min(2, int(160 * 1024 / S.lds_total)));
    int grid = int(std::min<int64_t>(n, int64_t(s.num_cu) * wg_per_cu));
    if (grid >= 8) grid &= ~7;
    int64_t chunk = n / (int64_t(grid) * 8);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, 8));     // measured: 8 is best, 1..64 within 3 %
    if (s.has_scan_chunk) chunk = std::max<int64_t>(1, s.scan_chunk);   // tuning knob
    S.grid = grid;
    S.chunk = int32_t(chunk);
    // fast paths: 512-thread workgroups, per-position loops unrolled ITS = 4 / 10 / 16 times (windows up to 2048 /
    // 5120 / 8192 bases); anything longer (up to 65535): generic 1024-thread kernel with runtime loops
    const int64_t need = (s.plan_maxwin + 511) / 512;
    S.its = need <= 4 ? 4 : need <= 10 ? 10 : need <= 16 ? 16 : 0;

    // narrow-counter form (scan8_kernel.h): K = 8, kmin <= 5 (shared prefix level), windows of at most 256 x 20 bases.
    // width 0 = adaptive (the default), 4 / 8 = fixed, anything else = off (scan_kernel.h's 16-bit form for everything)
    int width = FRISK_K8_WIDTH;
    if (s.has_k8_bits) width = s.k8_bits;
    // (decided by -w alone: rescued small scaffolds beyond the kernel's reach are handed on per window, see scan8_kernel.h)
    const bool narrow8 = k8 && s.kmin <= 5 && s.w <= 5120 && s.plan_maxwin <= 65535 && (width == 0 || width == 4 || width == 8);
    // K = 6, 7: the same kernel with 8-bit counters (a K-mer must occur 256 times in a window to wrap one)
    const bool narrow7 = (s.kmax == 6 || s.kmax == 7) && s.kmin <= s.kmax - 3 && s.w <= 5120 && s.plan_maxwin <= 65535 && width != 16;
    // (the per-max-mer IVOM dump of frisk_scan_ivom is written by scan_kernel.h's debug instantiation only)
    const bool narrow = (narrow8 || narrow7) && !s.want_ivom;

    if (s.plan_maxwin > 65535 || s.kmax > 8) {
        // windows beyond the 16-bit LDS counters, and every window at K > 8: 32-bit tables of all orders in a global scratch
        // slice per workgroup
        S.path = SCAN_PATH_BIG;
        S.big_grid = int(std::min<int64_t>(n, s.num_cu));
        return S;
    }
    S.form16 = scan16_form_of(s.kmax, S.its, debug, false);
    if (!narrow) {
        if (!k8 && !debug && !s.one_wg && s.plan_maxwin <= 5120 && S.lds_total <= 80 * 1024) {
            // K <= 7: the tables of a window take < 60 KB, so TWO independent 256-thread workgroups fit a CU.  The two waves of
            // a SIMD then belong to different windows in different stages, and the LDS phases of one overlap the VALU phases of
            // the other: measured -23 % (K = 7) and -26 % (K = 6) against one 512-thread workgroup with the same code.
            S.path = SCAN_PATH_TWO_WG;
            grid = int(std::min<int64_t>(n, int64_t(s.num_cu) * 2));
            if (grid >= 8) grid &= ~7;
            S.grid = grid;
            S.chunk = int32_t(std::max<int64_t>(1, std::min<int64_t>(n / (int64_t(grid) * 8), 8)));
            S.its = s.plan_maxwin <= 2048 ? 8 : 20;
            S.form16 = scan16_form_of(s.kmax, S.its, debug, true);
        } else {
            S.path = SCAN_PATH_16BIT;
        }
        return S;
    }

    // K = 8 default (scan8_kernel.h): narrow order-8 counters, three (4-bit) or two (8-bit) independent 256-thread
    // workgroups per CU.  A window with a max-mer that occurs 16+ (256+) times - poly-A, microsatellites, satellite arrays -
    // wraps a 4-bit (8-bit) counter; the kernel notices and hands it to the next wider form through a device-side list:
    //     4-bit bulk -> list 1 -> 8-bit -> list 2 -> 16-bit (scan_kernel.h)        or        8-bit bulk -> list 2 -> 16-bit.
    // Which width suits the bulk depends on the sequence, so (width 0) every 16th chunk of 8 windows is scanned with 4-bit
    // counters first, and the share of it that had to be handed on decides the width for the other fifteen.  All three
    // forms give the same bits for a window (same arithmetic; 16-bit only ever sees the windows that wrap 8 bits), so
    // results do not depend on the choice, on the grid, or on the candidate range.
    S.path = SCAN_PATH_NARROW;
    S.narrow8 = narrow8;
    S.small_w = s.w <= 2048;
    // chunks of 16 consecutive windows where the tables slide and the genome-side values travel through the ring (one window
    // in 16 is counted - and gathered - afresh; measured on the bench shard: 8: 6.71 ms, 12: 6.65, 16: 6.61, 24: 6.79), of 8 otherwise
    const bool can_slide = 2 * int64_t(s.inc) <= int64_t(s.w) - (s.kmax - 1) && !s.no_slide;
    // (chunks of 32 on long scans, FRISK8_CHUNK_LONG at c34d7fb: inside the noise, NOTES round 4)
    const int64_t chunk_cap = can_slide ? 16 : 8;
    int64_t chunk8 = std::max<int64_t>(1, std::min<int64_t>(n / (int64_t(s.num_cu) * 3 * 8), chunk_cap));
    // A SHORT scan (fewer than 2 x 16 windows per workgroup: BASELINE's C3, a rank's share of a small genome) is dealt statically in
    // TWO rounds of the launch's workgroups: chunks of ceil(n / (2 x workgroups)) windows, tables sliding and the ring inside a chunk.
    // Measured (tools/exp/c3_sweep.py, us per scan of the first n windows of the shard; window by window / the best chunk):
    // 1 500: 55 / 55 (1);  3 000: 87 / 86 (2);  6 000: 160 / 137 (4);  12 063: 303 / 243 (8);  24 000: 550 / 451 (16) - one round
    // of longer chunks puts every workgroup through the same stage at the same time (12 063 in chunks of 16: 323), chunks dealt by
    // counters cost such a scan an atomic's round trip per chunk (12 063 in chunks of 8: 269 dealt, 243 static).
    const int64_t wgs3 = int64_t(s.num_cu) * (narrow8 ? 3 : FRISK_K7_WPS);
    const bool short_scan = can_slide && n < wgs3 * 2 * 16 && !(s.flags & FRISK_SCAN_CHUNKS) && !s.has_scan_chunk;
    if (short_scan) chunk8 = std::max<int64_t>(1, (n + wgs3 * 2 - 1) / (wgs3 * 2));
    if (s.flags & FRISK_SCAN_CHUNKS) chunk8 = 8;
    if (s.has_scan_chunk) chunk8 = std::max<int64_t>(1, s.scan_chunk);
    S.can_slide = can_slide; S.short_scan = short_scan; S.chunk8 = chunk8;
    // inside a chunk the order-K table slides from window to window where two windows share more than half their bases
    // (2 inc updates instead of w - K + 1 and a cleared table; scan8_kernel.h)
    if (can_slide && chunk8 >= 2) S.slide_pp = int32_t((s.inc + 255) / 256);
    // the ring through which genome-side values travel from window to window (scan8_kernel.h): a copy of the genome table (one
    // base address for both) followed by one slice of 20 rows x 512 columns per workgroup launched.  Only the K = 8 / 4-bit
    // instantiations with the ring read it: launches whose windows slide, and the debug form
    if (narrow8 && (S.slide_pp > 0 || debug))
        S.ring_slices = std::min<int64_t>(std::max<int64_t>((n + chunk8 - 1) / chunk8, 1), int64_t(s.num_cu) * 4);
    const int64_t nchunks = (n + chunk8 - 1) / chunk8;
    S.nchunks = nchunks;
    // (the sample of the adaptive width: every 16th chunk, every 32nd or fewer of a long scan - a short launch runs at two thirds
    //  of a long one's rate, tools/exp/launch_size.py, and 12 000 windows tell the shares as well as 25 000
    //  ... and no more chunks than the launch has workgroups - one round: a second chunk for a few of them doubled its time)
    if (nchunks >= 64 * 32) S.sel_mod = int32_t(std::max<int64_t>(32, (nchunks + int64_t(s.num_cu) * 3 - 1) / (int64_t(s.num_cu) * 3)));
    // chunks dealt by counters (scan8_kernel.h) where a chunk is long enough to pay for the exchange: a short scan keeps the static deal
    const bool dealt = chunk8 >= 4 && !short_scan && !s.no_deal;
    S.dealt = dealt;
    int bulk = (width == 4 && narrow8) ? 4 : 8;
    bool side = false;              // 4-bit bulk with the side table (scan8_kernel.h, SIDE)
    const bool side_ok = narrow8 && !debug;
    const bool hinted = s.width_hint != 0 && s.hint_matches;
    if (narrow7) { /* 8-bit bulk, no sample */ }
    else if ((s.flags & (FRISK_SCAN_BITS4 | FRISK_SCAN_SIDE4)) && narrow8) { bulk = 4; side = (s.flags & FRISK_SCAN_SIDE4) && side_ok; }
    else if (width == 0 && !debug && hinted) { bulk = s.width_hint; side = s.hint_side && side_ok; }   // same batch, same geometry: the earlier sample still holds
    else if (width == 0 && !debug && nchunks >= 64 * S.sel_mod) {
        // the sample: every sel_mod-th chunk with 4-bit counters, then its own hand-overs; the verdict is taken on the device and all
        // three bulk forms are queued behind it (frisk_abi.hip, ScanRun::sample)
        S.sample = true;
        S.nsample = (nchunks + S.sel_mod - 1) / S.sel_mod;
        bulk = 4;                           // (what the launch shapes below assume until the verdict is read back)
        S.sel_mode = 2;
    }
    S.bulk = bulk; S.side = side;
    // The 4-bit bulk forms exist a second time, compiled for the lowest order 1 (scan8_kernel.h, KMIN1): K = 8 and kmin = 1 - the
    // default, and the reference's - take them, whatever width the bulk turns out to have (a launch of another width follows its own
    // rule: scan8_form_of); the debug instantiations, K = 6 and 7 and every other kmin keep the kernel that reads kmin as an argument,
    // and so does a scan that asks for it (FRISK_SCAN_GENERIC: the two are compared bit for bit).
    S.kmin1_form = narrow8 && s.kmin == 1 && !debug && !(s.flags & FRISK_SCAN_GENERIC);
    // the forms of the launches: a range launch slides where the schedule does, a hand-over launch walks a list and never slides
    Scan8Ask ask = Scan8Ask();
    ask.kmax = s.kmax; ask.kmin = s.kmin; ask.small_w = S.small_w; ask.kmin1_form = S.kmin1_form; ask.slides = S.slide_pp > 0;
    if (S.sample) {         // (no debug dump: the sample is not taken with one)
        Scan8Ask a = ask;
        a.bits = 4; a.sample = true;
        S.form_sample = scan8_form_of(a);
        a.sample = false;
        S.form_verdict[0] = scan8_form_of(a);
        a.side = true;
        S.form_verdict[1] = scan8_form_of(a);
        a.bits = 8; a.side = false;
        S.form_verdict[2] = scan8_form_of(a);
    } else {
        Scan8Ask a = ask;
        a.bits = bulk; a.debug = debug; a.side = side;
        S.form_bulk = scan8_form_of(a);
    }
    if (S.sample || bulk == 4) {
        Scan8Ask a = ask;
        a.bits = 8; a.debug = debug; a.listed = true;
        S.form_handover = scan8_form_of(a);
    }
    // The last sixteenth of a long scan goes to a second stream and starts when the kernels of the first fifteen are done:
    // it runs while their rows travel to the host (16 MB per 410 k windows: 0.36 ms that used to follow the scan).  The
    // cut is a multiple of 16 chunks: chunk numbering and the sample's stride stay aligned across it.
    const int64_t unit = chunk8 * S.sel_mod;
    int64_t cut = n;
    // (worth a second launch only when the rows' way to the host is long against a launch: 40 B x 128 K rows ~ 0.1 ms)
    if (!debug && !s.want_ivom && n >= (int64_t(1) << 17) && n >= 64 * unit && !s.one_segment) {
        cut = (n / unit - std::max<int64_t>(1, n / unit / 16)) * unit;
        // ... and the tail is a launch of its own: about a sixteenth of the windows is two chunks per workgroup - 1 616 chunks on 768
        // workgroups left a tenth of them a third chunk and the others idle (0.78 ms under the profiler for 0.40 ms of work).  So
        // the tail takes whole rounds: the largest number of chunks <= rounds x workgroups that the cut's alignment allows.
        const int64_t wgs = int64_t(s.num_cu) * (bulk == 4 ? 3 : 2);
        const int64_t tail_chunks = (n - cut + chunk8 - 1) / chunk8;
        if (tail_chunks >= wgs && !s.tail_any) {
            const int64_t rounds = (tail_chunks + wgs / 2) / wgs;
            // (a cut is a whole number of units - the kernels number a segment's chunks from its first candidate - and leaves a tail)
            cut = std::min((n / unit - 1) * unit, (n - rounds * wgs * chunk8 + unit - 1) / unit * unit);
        }
        if (cut <= 0 || cut >= n || cut % unit != 0) {
            S.error = "frisk_scan: row segments cut off a unit boundary";
            S.error_code = FRISK_E_STATE;
            return S;
        }
    }
    S.cut = cut;
    S.segments = cut < n ? 2 : 1;
    return S;
}
