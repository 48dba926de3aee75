// frisk_ctx.h - the context of the C ABI (include/frisk_hip.h) and what every host unit of it needs: the owners of device and
// page-locked memory, struct frisk_ctx with its sequence batches, the error path (fail, HIPC) and two small helpers.  The one
// definition of the context: frisk_abi.hip (context, phase A, scan) and frisk_seq.hip (sequences, FASTA) both include it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "frisk_hip.h"
#include "frisk_device.h"           // ScafDesc
#include "fasta_reader.h"           // NoInitAlloc
#include "scan_tiles.h"
#include "seq_pack2.h"              // Runs

// A device buffer (PINNED: a page-locked host block) that grows and is never shrunk; freed with its owner.  Not copyable: two
// owners would free it twice.  reserve(n) leaves room to grow, or as much as the caller says (`want` >= n elements).
template <typename T, bool PINNED = false>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;     // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n, size_t want = 0) {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = PINNED ? hipHostFree(p) : hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        if (!want) want = n + n / 8 + 64;
        void* q = nullptr;
        hipError_t e = PINNED ? hipHostMalloc(&q, want * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, want * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q);
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
};
template <typename T>
using PinBuf = DevBuf<T, true>;

struct frisk_ctx {
    int device = 0;
    int kmin = 1, kmax = 8;
    int64_t nprof = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms[9] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0};   // frisk_last_kernel_ms: scan, profile_add, pack / load, window vectors, score ranges, the panel, null sequences, explain, refine
    std::string err;

    // sequence batches: bat[cur] is the resident one; the other slot receives the next batch while the resident one is
    // being scanned (frisk_seq_stage / frisk_seq_commit)
    struct Batch {
        int32_t n_seq = 0;
        std::vector<int64_t> seq_off, seq_len;
        std::vector<std::string> seq_name;
        int64_t padded_len = 0;
        bool have_seq = false;
        DevBuf<uint8_t> d_ascii;
        DevBuf<uint32_t> d_codes, d_inv, d_low;
        // A TILED batch (frisk_fasta_load_shard) holds, per scaffold, only the bases one rank needs: the windows of its
        // candidate range plus the positions whose k-mers it counts.  "Sequences" of the layout above are then tiles.
        using Tile = ::Tile;    // scan_tiles.h
        int width_hint = 0, hint_w = 0, hint_inc = 0, hint_side = 0;   // counter width the last sampled scan of this batch chose (0: none yet)
        bool tiled = false;
        std::vector<Tile> tiles;
        int32_t tile_w = 0, tile_inc = 0;
        uint32_t tile_flags = 0;
        int64_t cand_begin = 0, cand_end = 0;       // the rank's range of the job's candidate numbering
        std::vector<std::string> g_name;            // all records of the FASTA
        std::vector<int64_t> g_len;
        // A STREAMED batch (frisk_seq_stage_2bit): the codes arrive in pieces on the copy stream; piece i - bitmap words
        // [piece_end[i-1], piece_end[i]) and their code words - is complete when piece_ev[i] has passed.  `streaming`: the compute
        // stream has not waited for them yet (frisk_profile_add follows the pieces one by one; anything else waits for the last).
        std::vector<int64_t> piece_end;
        std::vector<hipEvent_t> piece_ev;
        bool streaming = false;
        DevBuf<int64_t> d_runs;                     // the run lists of the two masks and of the PADs, as uploaded
        // frisk_fasta_load packs on the host and keeps the 0.25 B/base form until the next load: frisk_seq_export_2bit (the CLI's
        // sequence cache) hands it out without touching the device
        std::vector<uint32_t, frisk_fasta::NoInitAlloc<uint32_t>> h_codes;
        frisk_pack2::Runs h_runs;
        bool have_host2 = false;
        PinBuf<int64_t> h_pads;                     // page-locked: the PAD runs on their way to the device
        ~Batch() { for (hipEvent_t e : piece_ev) (void)hipEventDestroy(e); }
    };
    Batch bat[2];
    int cur = 0;
    Batch& b() { return bat[cur]; }
    const Batch& b() const { return bat[cur]; }
    hipStream_t copy_stream = nullptr;      // uploads + packing of the staged batch
    // h2d(): pageable host memory goes through these page-locked pieces (4 worker threads x 2), not through the runtime's own staging
    static constexpr int PIN_N = 8;
    static constexpr size_t PIN_BYTES = size_t(16) << 20;
    PinBuf<unsigned char> pin_buf[PIN_N];
    hipEvent_t pin_ev[PIN_N] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool pin_busy[PIN_N] = {false, false, false, false, false, false, false, false};
    hipStream_t tail_stream = nullptr;      // frisk_scan: the last sixteenth of a long scan, while the rows of the rest go to the host
    hipEvent_t ev_fork = nullptr, ev_tail_kernels = nullptr, ev_tail_done = nullptr;
    hipEvent_t staged_ev = nullptr;         // recorded behind the staged batch's last operation
    hipEvent_t slot_free_ev = nullptr;      // recorded on `stream` at every commit: everything queued there before it may still read the
    bool slot_ev_set = false;               // batch slot that the NEXT stage overwrites (profile kernels and scans are asynchronous)
    bool staged = false;

    // profile
    DevBuf<int64_t> d_raw, d_cnt, d_sym;
    DevBuf<double> d_ig, d_logtab, d_logtab64, d_logtab32, d_rctab;
    DevBuf<int64_t> d_ovf_list, d_ovf_list2;   // windows handed from 4-bit to 8-bit counters, and from there to the 16-bit form
    uint64_t ig_gen = 1, ring_gen = 0;         // the genome table's generation, and the one whose copy heads d_ig_ring
    DevBuf<double> d_ig_ring;                  // scan8_kernel: per-workgroup ring of genome-side values by position (40 KB each at 20 positions per lane)
    DevBuf<unsigned int> d_verdict;            // the adaptive width's verdict, written on the device by scan8_decide_kernel: {form, handed, would-have, scored}
    DevBuf<unsigned int> d_ovf_count;          // SCAN_CNT_TOTAL counters, SCAN_CNT_SEGMENT per row segment (ScanCounter, scan_params.h): the lists' lengths, the sample's counts, the launches' chunk queues
    int64_t scan_stat[6] = {0, 0, 0, 0, 0, 0}; // most recent scan: counter width of the bulk launch, windows handed 4->8, ->16, row segments,
                                               // 1 = the bulk launch had the side table for period-4 max-mers beside its 4-bit counters,
                                               // 1 = the 4-bit bulk launch was the kernel compiled for kmin = 1
    DevBuf<uint32_t> d_big;      // 32-bit tables of the long-window path (scan_big_kernel.h), one slice per workgroup
    DevBuf<int64_t> d_meta;          // {totalLen, exMax, nnTotal} of the finalised profile, on the device
    PinBuf<int64_t> h_meta;          // page-locked mirror, valid after the stream has been synchronised
    bool profile_final = false;
    // the panel of frisk_score_ranges_panel: snapshots of finalised genome-side tables, FRISK_PANEL_TILE to a block of
    // [code][FRISK_PANEL_TILE] doubles (panel_kernels.h); a block is allocated when its first slot is pushed
    DevBuf<double> panel_tile[FRISK_PANEL_MAX / FRISK_PANEL_TILE];
    int32_t panel_n = 0;
    bool ms_pending[3] = {false, false, false};     // events recorded, elapsed time not read yet (frisk_last_kernel_ms)
    hipEvent_t evp0 = nullptr, evp1 = nullptr;      // profile_add kernel
    hipEvent_t evn0 = nullptr, evn1 = nullptr;      // frisk_seq_null's kernels (created by its first call)

    // scan plan + outputs
    DevBuf<ScafDesc> d_desc;
    std::vector<ScafDesc> h_desc;
    int32_t plan_w = -1, plan_inc = -1;
    uint32_t plan_flags = 0;
    int64_t plan_ncand = 0;
    int64_t plan_maxwin = 0;
    DevBuf<int32_t> o_seq;
    DevBuf<int64_t> o_start, o_stop, o_meta;
    DevBuf<uint32_t> o_status, o_counts;
    DevBuf<double> o_kld, o_gc, o_pi, o_si, o_cri, o_sw, o_sg, o_ivom;
    // a SHORT scan's row columns sit in one device block and travel to the host as ONE copy into this page-locked block (the
    // runtime spaces small device-to-host copies ~14 us apart: seven of them were 0.1 ms behind a 0.3 ms scan)
    DevBuf<double> o_block;
    PinBuf<unsigned char> h_block;
    double* want_ivom = nullptr;     // frisk_scan_ivom: host buffer of the per-max-mer dump requested from the next debug scan
};

inline int fail(frisk_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPC(ctx, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((ctx), FRISK_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline int grid_for(int64_t items, int per_block, int max_blocks) {
    int64_t b = (items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return int(b);
}

// A streamed batch (frisk_seq_stage_2bit) whose pieces the compute stream has not followed: wait, on the device, for the last
inline int settle_stream(frisk_ctx* c) {
    frisk_ctx::Batch& B = c->b();
    if (!B.streaming) return FRISK_OK;
    if (!B.piece_end.empty()) HIPC(c, hipStreamWaitEvent(c->stream, B.piece_ev[B.piece_end.size() - 1], 0));
    B.streaming = false;
    return FRISK_OK;
}
