// frisk_seq.hip - the sequence half of the C ABI declared in include/frisk_hip.h: how a batch gets onto the device (ASCII, packed, the
// 0.25 B/base form; loaded into the resident slot, or staged into the other one and committed), the FASTA entry points with the
// window-tile shard loaders, the batches generated on the device (synthetic scaffolds; null sequences from the finalised profile's
// Markov chain, null_kernels.h), and a batch's way back to the host.  The context is frisk_ctx.h's; its creation, phase A and the scan
// are in frisk_abi.hip.  gfx950 (MI355X) only.  Build: see __graft_entry__.build_hip().
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "frisk_ctx.h"
#include "seq_kernels.h"
#include "synth_kernel.h"
#include "null_kernels.h"
#include "fasta_index.h"
#include "fasta_pack2.h"

namespace {

// threads of a host-side parse or pack: the hardware's, `cap` at the most, of which a rank takes one `share`-th (the ranks of a job
// parse the same file at the same time, normally on one node)
int host_threads(unsigned cap, int share = 1) {
    const unsigned hw = std::thread::hardware_concurrency();
    return int(std::max(1u, std::min(cap, (hw ? hw : 1u) / unsigned(share))));
}

// a malloc'ed copy for the caller to frisk_free (an empty array still gets a pointer)
bool give(const void* src, size_t bytes, void** out) {
    *out = std::malloc(std::max<size_t>(bytes, 16));
    if (!*out) return false;
    if (bytes) std::memcpy(*out, src, bytes);
    return true;
}

// the run lists of the two masks as malloc'ed arrays of [begin, end) pairs: both or neither
bool give_runs(const std::vector<int64_t>& inv, const std::vector<int64_t>& low, int64_t** inv_runs, int64_t* n_inv, int64_t** low_runs,
               int64_t* n_low) {
    *n_inv = int64_t(inv.size() / 2);
    *n_low = int64_t(low.size() / 2);
    if (!give(inv.data(), inv.size() * sizeof(int64_t), reinterpret_cast<void**>(inv_runs))) return false;
    if (!give(low.data(), low.size() * sizeof(int64_t), reinterpret_cast<void**>(low_runs))) { std::free(*inv_runs); *inv_runs = nullptr; return false; }
    return true;
}

// a message (or a name) into a caller's buffer of `cap` bytes, cut to fit
void say(char* dst, int32_t cap, const std::string& m) {
    if (dst && cap > 0) { std::strncpy(dst, m.c_str(), size_t(cap) - 1); dst[cap - 1] = 0; }
}

// layout of a batch in padded coordinates (frisk_device.h): scaffold s at [off, off+len), then at least one PAD; into `slot`, or into
// the resident one.  The arguments are checked before the batch is touched: a refused load or stage leaves the batch in the slot as it was.
int layout_batch(frisk_ctx* c, const int64_t* lens, int32_t n_seq, frisk_ctx::Batch* slot = nullptr) {
    frisk_ctx::Batch& B = slot ? *slot : c->b();
    if (n_seq < 0) return fail(c, FRISK_E_ARG, "n_seq < 0");
    for (int32_t s = 0; s < n_seq; ++s)
        if (lens[s] < 0) return fail(c, FRISK_E_ARG, "negative scaffold length");
    // The loaders refill the RESIDENT slot on the compute stream: the pieces of a streamed upload into it may still be in flight on
    // the copy stream, so the compute stream waits for the last one (on the device) before anything writes the slot.  The stage
    // forms fill the other slot on the copy stream, which is ordered behind its own pieces already.
    if (&B == &c->b()) {
        const int rc = settle_stream(c);
        if (rc) return rc;
    }
    B.seq_off.assign(size_t(n_seq), 0);
    B.seq_len.assign(lens, lens + n_seq);
    B.seq_name.assign(size_t(n_seq), std::string());
    int64_t pos = 0;
    for (int32_t s = 0; s < n_seq; ++s) {
        B.seq_off[size_t(s)] = pos;
        pos += lens[s] + 1;                       // at least one PAD position after every scaffold
    }
    B.padded_len = (pos + 31) / 32 * 32;
    if (B.padded_len == 0) B.padded_len = 32;
    B.n_seq = n_seq;
    B.have_seq = false;
    B.width_hint = 0;
    B.tiled = false;
    B.tiles.clear(); B.g_name.clear(); B.g_len.clear();
    B.streaming = false;        // (piece_end is kept: frisk_seq_stage_2bit looks at the slot's previous upload; the resident slot was settled above)
    if (B.have_host2) {
        B.have_host2 = false;
        decltype(B.h_codes)().swap(B.h_codes);
        B.h_runs = frisk_pack2::Runs();
    }
    return FRISK_OK;
}

// packed arrays of a batch: allocate, and mark the words past the batch.  Without arguments: the resident batch, on the compute stream
int alloc_packed(frisk_ctx* c, frisk_ctx::Batch* slot = nullptr, hipStream_t st = nullptr) {
    frisk_ctx::Batch& B = slot ? *slot : c->b();
    if (!slot) st = c->stream;
    const size_t w32 = size_t(B.padded_len / 32);
    HIPC(c, B.d_codes.reserve(2 * w32 + 8));
    HIPC(c, B.d_inv.reserve(w32 + 8));
    HIPC(c, B.d_low.reserve(w32 + 8));
    // tail words past the batch: codes 0, inv/low all ones (= PAD), so a run can never extend past the end
    HIPC(c, hipMemsetAsync(B.d_codes.p + 2 * w32, 0, 8 * sizeof(uint32_t), st));
    HIPC(c, hipMemsetAsync(B.d_inv.p + w32, 0xFF, 8 * sizeof(uint32_t), st));
    HIPC(c, hipMemsetAsync(B.d_low.p + w32, 0xFF, 8 * sizeof(uint32_t), st));
    return FRISK_OK;
}

// ASCII -> packed, on stream `st`, no host synchronisation
int enqueue_pack(frisk_ctx* c, frisk_ctx::Batch& B, hipStream_t st) {
    const int64_t w32 = B.padded_len / 32;
    if (w32 > 0)
        pack_kernel<<<grid_for(w32, 256, c->num_cu * 8), 256, 0, st>>>(B.d_ascii.p, w32, B.d_codes.p, B.d_inv.p, B.d_low.p);
    HIPC(c, hipGetLastError());
    return FRISK_OK;
}

// common tail of the synchronous loaders: what they queued on the compute stream behind ev0 has run when this returns, timed
int finish_timed_load(frisk_ctx* c) {
    HIPC(c, hipEventRecord(c->ev1, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->ms[2] = ms;
    c->b().have_seq = true;
    c->plan_w = -1;
    return FRISK_OK;
}

// common tail of frisk_seq_load / frisk_seq_synth / the shard loaders: pack the resident batch, timed, synchronous
int run_pack(frisk_ctx* c) {
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    if (int rc = enqueue_pack(c, c->b(), c->stream)) return rc;
    return finish_timed_load(c);
}

// Host -> device copy on stream `st`.  Page-locked sources go straight to the copy engine (asynchronous).  A large PAGEABLE source -
// the parser's buffer of a multi-gigabase FASTA, a Python bytes object - would be staged by the runtime at ~3 GB/s (measured: 1.03 s
// for the 3.3 Gb assembly); here four threads copy it through page-locked 16 MB pieces of the context's, two per thread, and the
// copy engine follows them at PCIe rate.  On return every byte of `src` has been read (the DMAs may still be in flight, from the
// context's buffers).
int h2d(frisk_ctx* c, void* dst, const void* src, size_t n, hipStream_t st) {
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();                           // (an unregistered host pointer is reported as an error: expected)
    if (pinned || n < 4 * frisk_ctx::PIN_BYTES) {
        HIPC(c, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st));
        return FRISK_OK;
    }
    for (int i = 0; i < frisk_ctx::PIN_N; ++i) {
        if (!c->pin_buf[i].p) {
            HIPC(c, c->pin_buf[i].reserve(frisk_ctx::PIN_BYTES, frisk_ctx::PIN_BYTES));
            HIPC(c, hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
        }
    }
    constexpr int WORKERS = frisk_ctx::PIN_N / 2;
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&](int wk) {
        if (hipSetDevice(c->device) != hipSuccess) { bad = 1; return; }
        for (int it = 0; !bad; ++it) {
            const size_t off = next.fetch_add(1) * frisk_ctx::PIN_BYTES;
            if (off >= n) break;
            const int b = wk * 2 + (it & 1);
            if (c->pin_busy[b] && hipEventSynchronize(c->pin_ev[b]) != hipSuccess) { bad = 1; break; }   // the DMA that last read this piece
            const size_t len = std::min(frisk_ctx::PIN_BYTES, n - off);
            std::memcpy(c->pin_buf[b].p, static_cast<const char*>(src) + off, len);
            if (hipMemcpyAsync(static_cast<char*>(dst) + off, c->pin_buf[b].p, len, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipEventRecord(c->pin_ev[b], st) != hipSuccess) { bad = 1; break; }
            c->pin_busy[b] = true;
        }
    };
    std::vector<std::thread> th;
    for (int wk = 1; wk < WORKERS; ++wk) th.emplace_back(work, wk);
    work(0);
    for (auto& t : th) t.join();
    if (bad) return fail(c, FRISK_E_HIP, "host-to-device copy through the page-locked staging buffers failed");
    return FRISK_OK;
}

// ASCII scaffolds -> B.d_ascii on stream `st` (asynchronous for page-locked sources)
int enqueue_ascii_upload(frisk_ctx* c, frisk_ctx::Batch& B, const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq,
                         hipStream_t st) {
    HIPC(c, B.d_ascii.reserve(size_t(B.padded_len)));
    // PAD everywhere first: the gaps between scaffolds and the tail.  (One memset of the whole buffer costs 0.1 ms per 400 MB.)
    HIPC(c, hipMemsetAsync(B.d_ascii.p, FRISK_PAD_BYTE, size_t(B.padded_len), st));
    for (int32_t s = 0; s < n_seq; ++s)
        if (lens[s] > 0) {
            const int rc = h2d(c, B.d_ascii.p + B.seq_off[size_t(s)], seqs[s], size_t(lens[s]), st);
            if (rc) return rc;
        }
    return FRISK_OK;
}

// The stage forms fill the slot that is NOT resident, on the copy stream, between these two.  begin_stage: work queued on the compute
// stream before the last commit may still be reading that slot, so the copy stream waits for it (on the device) before layout_batch
// touches the slot.  end_stage: the event behind the staged batch's last operation (`pieces`: and an event behind each piece of its
// codes, which frisk_profile_add may follow one by one); frisk_seq_commit may follow.
int begin_stage(frisk_ctx* c, const int64_t* lens, int32_t n_seq, frisk_ctx::Batch*& B) {
    HIPC(c, hipSetDevice(c->device));
    B = &c->bat[c->cur ^ 1];
    c->staged = false;
    if (c->slot_ev_set) HIPC(c, hipStreamWaitEvent(c->copy_stream, c->slot_free_ev, 0));
    return layout_batch(c, lens, n_seq, B);
}
int end_stage(frisk_ctx* c, frisk_ctx::Batch& B, bool pieces = false) {
    HIPC(c, hipEventRecord(c->staged_ev, c->copy_stream));
    B.streaming = pieces;
    c->staged = true;
    return FRISK_OK;
}

// the resident batch's three packed arrays to the host; they are there on return
int d2h_packed(frisk_ctx* c, uint32_t* codes, uint32_t* inv, uint32_t* low) {
    const frisk_ctx::Batch& B = c->b();
    const size_t w32 = size_t(B.padded_len / 32);
    HIPC(c, hipMemcpyAsync(codes, B.d_codes.p, 2 * w32 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(inv, B.d_inv.p, w32 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(low, B.d_low.p, w32 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return FRISK_OK;
}

// What the two shard loaders share.  The checks come first in both, ahead of the file.  Once the records' lengths are known: this
// rank's tiles, and the resident slot laid out for what each keeps resident ("sequences" of the layout are tiles: seq_len[t] bases
// from tiles[t].base0 on).  The batch is not `tiled` before finish_tiled.
int check_shard(frisk_ctx* c, int32_t w, int32_t inc, int32_t rank, int32_t world) {
    if (w < 1 || inc < 1) return fail(c, FRISK_E_ARG, "window length and increment must be >= 1");
    if (world < 1 || rank < 0 || rank >= world) return fail(c, FRISK_E_ARG, "rank outside [0, world)");
    return FRISK_OK;
}
int plan_tiled_batch(frisk_ctx* c, const std::vector<int64_t>& lens, int32_t w, int32_t inc, uint32_t flags, int32_t rank, int32_t world) {
    int64_t c0 = 0, c1 = 0;
    std::vector<Tile> tiles = plan_tiles(lens, w, inc, (flags & FRISK_SCAN_SCAFFOLDS_ALL) != 0, c->kmax, rank, world, c0, c1);
    std::vector<int64_t> tlen(tiles.size());
    for (size_t t = 0; t < tiles.size(); ++t) tlen[t] = tile_end(tiles[t], w, inc, c->kmax) - tiles[t].base0;
    if (int rc = layout_batch(c, tlen.data(), int32_t(tiles.size()))) return rc;
    frisk_ctx::Batch& B = c->b();
    B.tiles.swap(tiles);
    B.tile_w = w; B.tile_inc = inc; B.tile_flags = flags & FRISK_SCAN_SCAFFOLDS_ALL;
    B.cand_begin = c0; B.cand_end = c1;
    return FRISK_OK;
}

// common tail of the two shard loaders: the tiles' ASCII is on the device; pack it and remember what the tiles are tiles of
int finish_tiled(frisk_ctx* c, const std::vector<std::string>& names, const std::vector<int64_t>& lens, int32_t* n_seq_out,
                 int64_t* total_len_out, int64_t* cand_begin, int64_t* cand_end) {
    frisk_ctx::Batch& B = c->b();
    if (int rc = alloc_packed(c)) return rc;
    if (int rc = run_pack(c)) return rc;
    B.tiled = true;
    B.g_name = names;
    B.g_len = lens;
    int64_t total = 0;
    for (int64_t v : lens) total += v;
    if (n_seq_out) *n_seq_out = int32_t(lens.size());
    if (total_len_out) *total_len_out = total;
    if (cand_begin) *cand_begin = B.cand_begin;
    if (cand_end) *cand_end = B.cand_end;
    return FRISK_OK;
}

// one mask of a streamed batch: zero the bitmap, then the caller's run list (or the caller's dense bitmap), then the PADs
int enqueue_mask(frisk_ctx* c, frisk_ctx::Batch& B, uint32_t* d_bits, const int64_t* runs, int64_t n_runs, int64_t* d_runs,
                 const int64_t* d_pads, int64_t n_pads, hipStream_t st) {
    const size_t w32 = size_t(B.padded_len / 32);
    if (n_runs < 0) {               // dense: P / 32 words in the library's layout (real bases only; PADs are added here)
        int rc = h2d(c, d_bits, runs, w32 * 4, st);
        if (rc) return rc;
    } else if (size_t(n_runs) * 16 > w32 * 4 + (size_t(1) << 20)) {
        // more bytes of runs than of bitmap (a sequence that changes case every few bases): expand here, upload densely
        std::vector<uint32_t> bits(w32, 0u);
        for (int64_t r = 0; r < n_runs; ++r)
            for (int64_t p = runs[2 * r]; p < runs[2 * r + 1]; ++p) bits[size_t(p >> 5)] |= 0x80000000u >> (p & 31);
        int rc = h2d(c, d_bits, bits.data(), w32 * 4, st);
        if (rc) return rc;
        HIPC(c, hipStreamSynchronize(st));              // (`bits` is a local)
    } else {
        HIPC(c, hipMemsetAsync(d_bits, 0, w32 * 4, st));
        if (n_runs > 0) {
            int rc = h2d(c, d_runs, runs, size_t(n_runs) * 16, st);
            if (rc) return rc;
            expand_runs_kernel<<<grid_for(n_runs, 4, c->num_cu * 16), 256, 0, st>>>(d_runs, n_runs, d_bits);
            HIPC(c, hipGetLastError());
        }
    }
    expand_runs_kernel<<<grid_for(n_pads, 4, c->num_cu * 16), 256, 0, st>>>(d_pads, n_pads, d_bits);
    HIPC(c, hipGetLastError());
    return FRISK_OK;
}

// the 0.25 B/base form of batch B (laid out by the caller) onto the device, on stream `st`: masks from the run lists, the codes
// in pieces with an event behind each
int upload_2bit(frisk_ctx* c, frisk_ctx::Batch& B, const uint32_t* codes, const int64_t* inv_runs, int64_t n_inv,
                const int64_t* low_runs, int64_t n_low, int64_t piece_bases, hipStream_t st) {
    const int64_t P = B.padded_len;
    const int32_t n_seq = B.n_seq;
    for (const auto& L : {std::make_pair(inv_runs, n_inv), std::make_pair(low_runs, n_low)})
        for (int64_t r = 0; r < L.second; ++r)
            if (L.first[2 * r] < 0 || L.first[2 * r] > L.first[2 * r + 1] || L.first[2 * r + 1] > P)
                return fail(c, FRISK_E_ARG, "frisk_seq_stage_2bit: a run outside the batch");
    int rc = alloc_packed(c, &B, st);
    if (rc) return rc;
    // PAD runs: the position behind every scaffold, and the batch's tail (inv AND low, frisk_device.h); adjacent ones merged
    // (the page-locked buffer they travel from may still feed the copy of this slot's previous upload: wait for that one)
    if (!B.piece_end.empty() && !B.piece_ev.empty()) HIPC(c, hipEventSynchronize(B.piece_ev[std::min(B.piece_end.size(), B.piece_ev.size()) - 1]));
    std::vector<int64_t> pads;
    for (int32_t s = 0; s < n_seq; ++s) frisk_pack2::push_run(pads, B.seq_off[size_t(s)] + B.seq_len[size_t(s)], B.seq_off[size_t(s)] + B.seq_len[size_t(s)] + 1);
    {
        const int64_t tail = n_seq > 0 ? B.seq_off[size_t(n_seq) - 1] + B.seq_len[size_t(n_seq) - 1] + 1 : 0;
        if (tail < P) frisk_pack2::push_run(pads, tail, P);
    }
    const int64_t n_pads = int64_t(pads.size() / 2);
    const size_t need = 2 * size_t(std::max<int64_t>(n_inv, 0) + std::max<int64_t>(n_low, 0) + n_pads) + 8;
    HIPC(c, B.d_runs.reserve(need));
    int64_t* d_pads = B.d_runs.p;
    int64_t* d_inv_runs = d_pads + 2 * n_pads;
    int64_t* d_low_runs = d_inv_runs + 2 * std::max<int64_t>(n_inv, 0);
    HIPC(c, B.h_pads.reserve(pads.size(), pads.size() + pads.size() / 4 + 16));
    std::memcpy(B.h_pads.p, pads.data(), pads.size() * sizeof(int64_t));
    HIPC(c, hipMemcpyAsync(d_pads, B.h_pads.p, pads.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    rc = enqueue_mask(c, B, B.d_inv.p, inv_runs, n_inv, d_inv_runs, d_pads, n_pads, st);
    if (rc) return rc;
    rc = enqueue_mask(c, B, B.d_low.p, low_runs, n_low, d_low_runs, d_pads, n_pads, st);
    if (rc) return rc;
    // the codes, piece by piece: an event behind each, so that phase A can follow the copies (frisk_profile_add)
    const int64_t w32 = P / 32;
    // default: 256 Mbases = 64 MB of codes (measured on the whole C5 shape, ms per streamed job: pieces of 8 MB 71.6, 16 MB 69.2,
    // 32 MB 67.5, 64 MB 66.6, 128 MB 66.5 - the copy engine leaves ~20 us between two copies, the last piece's profile kernel
    // is what follows the upload: tools/exp/piece_sweep.py)
    int64_t piece_words = (piece_bases ? piece_bases : (int64_t(1) << 28)) / 32;
    if (piece_words < 1) piece_words = 1;
    const int64_t n_pieces = std::max<int64_t>(1, (w32 + piece_words - 1) / piece_words);
    if (n_pieces > 4096) piece_words = (w32 + 4095) / 4096;
    B.piece_end.clear();
    for (int64_t a = 0; a < w32; a += piece_words) {
        const int64_t b = std::min(w32, a + piece_words);
        rc = h2d(c, B.d_codes.p + 2 * a, codes + 2 * a, size_t(b - a) * 8, st);
        if (rc) return rc;
        const size_t i = B.piece_end.size();
        if (B.piece_ev.size() <= i) {
            hipEvent_t ev = nullptr;
            HIPC(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            B.piece_ev.push_back(ev);
        }
        HIPC(c, hipEventRecord(B.piece_ev[i], st));
        B.piece_end.push_back(b);
    }
    return FRISK_OK;
}

}  // namespace

extern "C" {

// ---- loaders of the resident slot: synchronous, timed (frisk_last_kernel_ms(2)) ---------------------------------------------
int frisk_seq_load(frisk_ctx* c, const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq) {
    if (!c) return FRISK_E_ARG;
    if (n_seq > 0 && (!seqs || !lens)) return fail(c, FRISK_E_ARG, "null sequence table");
    HIPC(c, hipSetDevice(c->device));
    int rc = layout_batch(c, lens, n_seq);
    if (rc) return rc;
    if (n_seq <= 64) {
        rc = enqueue_ascii_upload(c, c->b(), seqs, lens, n_seq, c->stream);
        if (rc) return rc;
    } else {            // many small scaffolds: assemble once on the host, one copy
        HIPC(c, c->b().d_ascii.reserve(size_t(c->b().padded_len)));
        std::vector<uint8_t> stage(size_t(c->b().padded_len), uint8_t(FRISK_PAD_BYTE));
        for (int32_t s = 0; s < n_seq; ++s)
            if (lens[s] > 0) std::memcpy(stage.data() + c->b().seq_off[size_t(s)], seqs[s], size_t(lens[s]));
        rc = h2d(c, c->b().d_ascii.p, stage.data(), stage.size(), c->stream);
        if (rc) return rc;
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    rc = alloc_packed(c);
    if (rc) return rc;
    return run_pack(c);
}

int frisk_fasta_pack_2bit(const char* path, int32_t* n_seq, int64_t** lens, uint32_t** codes, int64_t* n_code_words, int64_t** inv_runs,
                          int64_t* n_inv, int64_t** low_runs, int64_t* n_low) {
    if (!path || !n_seq || !lens || !codes || !n_code_words || !inv_runs || !n_inv || !low_runs || !n_low) return FRISK_E_ARG;
    frisk_fasta::Records rec;
    frisk_fasta::CodeVec packed;
    frisk_pack2::Runs R;
    std::string err;
    if (!frisk_fasta::parse_pack(path, rec, packed, R, err, host_threads(32))) return FRISK_E_ARG;
    void *pl = nullptr, *pc = nullptr;
    if (!(give(rec.lens.data(), rec.lens.size() * 8, &pl) && give(packed.data(), packed.size() * 4, &pc) &&
          give_runs(R.inv, R.low, inv_runs, n_inv, low_runs, n_low))) { std::free(pl); std::free(pc); return FRISK_E_HIP; }
    *n_seq = int32_t(rec.lens.size());
    *lens = static_cast<int64_t*>(pl); *codes = static_cast<uint32_t*>(pc); *n_code_words = int64_t(packed.size());
    return FRISK_OK;
}

int frisk_fasta_digest(const char* path, int32_t* n_seq, int64_t* total_len, uint64_t* digest) {
    if (!path) return FRISK_E_ARG;
    frisk_fasta::Records rec;
    std::string err;
    if (!frisk_fasta::parse(path, rec, err)) return FRISK_E_ARG;
    uint64_t h = 1469598103934665603ull;                       // FNV-1a over name \0 sequence \0, record after record
    auto eat = [&h](const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; } };
    const uint8_t zero = 0;
    int64_t total = 0, off = 0;
    for (size_t r = 0; r < rec.lens.size(); ++r) {
        eat(reinterpret_cast<const uint8_t*>(rec.names[r].data()), rec.names[r].size());
        eat(&zero, 1);
        eat(rec.stage.data() + off, size_t(rec.lens[r]));
        eat(&zero, 1);
        if (rec.stage[size_t(off + rec.lens[r])] != FRISK_PAD_BYTE) return FRISK_E_STATE;       // the PAD behind every record
        off += rec.lens[r] + 1;
        total += rec.lens[r];
    }
    if (size_t(off) != rec.stage.size()) return FRISK_E_STATE;
    if (n_seq) *n_seq = int32_t(rec.lens.size());
    if (total_len) *total_len = total;
    if (digest) *digest = h;
    return FRISK_OK;
}

int frisk_fasta_load_shard(frisk_ctx* c, const char* path, int32_t w, int32_t inc, uint32_t flags, int32_t rank, int32_t world,
                           int32_t* n_seq_out, int64_t* total_len_out, int64_t* cand_begin, int64_t* cand_end) {
    if (!c || !path) return FRISK_E_ARG;
    if (int rc = check_shard(c, w, inc, rank, world)) return rc;
    frisk_fasta::Records rec;
    std::string err;
    if (!frisk_fasta::parse(path, rec, err, host_threads(~0u, world))) return fail(c, FRISK_E_ARG, err);
    HIPC(c, hipSetDevice(c->device));
    if (int rc = plan_tiled_batch(c, rec.lens, w, inc, flags, rank, world)) return rc;
    frisk_ctx::Batch& B = c->b();
    // the rank's tiles straight from the parser's buffer into the batch layout on the device (no second host copy of them):
    // PAD everywhere first, then one upload per tile
    std::vector<int64_t> rec_off(rec.lens.size());          // where record s starts in the parser's buffer
    int64_t pos = 0;
    for (size_t s = 0; s < rec.lens.size(); ++s) { rec_off[s] = pos; pos += rec.lens[s] + 1; }
    std::vector<const uint8_t*> src(B.tiles.size());
    for (size_t t = 0; t < src.size(); ++t) src[t] = rec.stage.data() + rec_off[size_t(B.tiles[t].scaf)] + B.tiles[t].base0;
    if (int rc = enqueue_ascii_upload(c, B, src.data(), B.seq_len.data(), B.n_seq, c->stream)) return rc;
    HIPC(c, hipStreamSynchronize(c->stream));          // (the parser's buffer goes away with this call)
    return finish_tiled(c, rec.names, rec.lens, n_seq_out, total_len_out, cand_begin, cand_end);
}

// ---- the same from a seek index: the rank maps the file and copies the bytes of ITS tiles, nothing else (fasta_index.h) ----
int frisk_fasta_index_build(const char* fasta_path, const char* index_path, int32_t* n_seq, char* why, int32_t why_cap) {
    if (!fasta_path || !index_path) return FRISK_E_ARG;
    say(why, why_cap, "");
    frisk_fasta::MappedFile f(fasta_path);
    if (!f.good) { say(why, why_cap, std::string("cannot open FASTA file: ") + fasta_path); return FRISK_E_ARG; }
    std::vector<frisk_fasta::FaiEntry> idx;
    std::string msg;
    if (!frisk_fasta::build_index(f, idx, msg)) { say(why, why_cap, msg); return FRISK_E_INDEX; }
    if (!frisk_fasta::write_index(index_path, f, idx, msg)) { say(why, why_cap, msg); return FRISK_E_ARG; }
    if (n_seq) *n_seq = int32_t(idx.size());
    return FRISK_OK;
}

int frisk_fasta_index_read(const char* fasta_path, const char* index_path, int32_t seq_index, int64_t pos0, int64_t n, uint8_t* out,
                           int32_t* n_seq, int64_t* seq_len, char* name, int32_t name_cap, char* why, int32_t why_cap) {
    if (!fasta_path || !index_path) return FRISK_E_ARG;
    say(why, why_cap, "");
    frisk_fasta::MappedFile f(fasta_path);
    if (!f.good) { say(why, why_cap, std::string("cannot open FASTA file: ") + fasta_path); return FRISK_E_ARG; }
    std::vector<frisk_fasta::FaiEntry> idx;
    std::string msg;
    if (!frisk_fasta::read_index(index_path, f, idx, msg)) { say(why, why_cap, msg); return FRISK_E_INDEX; }
    if (n_seq) *n_seq = int32_t(idx.size());
    if (seq_index < 0) return FRISK_OK;                 // (the count alone)
    if (size_t(seq_index) >= idx.size()) { say(why, why_cap, "record index out of range"); return FRISK_E_ARG; }
    const frisk_fasta::FaiEntry& r = idx[size_t(seq_index)];
    if (seq_len) *seq_len = r.len;
    say(name, name_cap, r.name);
    if (n > 0) {
        if (!out || pos0 < 0 || pos0 + n > r.len) { say(why, why_cap, "range outside the record"); return FRISK_E_ARG; }
        frisk_fasta::read_range(f, r, pos0, n, out);
    }
    return FRISK_OK;
}

int frisk_fasta_load_shard_indexed(frisk_ctx* c, const char* path, const char* index_path, int32_t w, int32_t inc, uint32_t flags,
                                   int32_t rank, int32_t world, int32_t* n_seq_out, int64_t* total_len_out, int64_t* cand_begin,
                                   int64_t* cand_end) {
    if (!c || !path || !index_path) return FRISK_E_ARG;
    if (int rc = check_shard(c, w, inc, rank, world)) return rc;
    frisk_fasta::MappedFile f(path);
    if (!f.good) return fail(c, FRISK_E_ARG, std::string("cannot open FASTA file: ") + path);
    std::vector<frisk_fasta::FaiEntry> idx;
    std::string msg;
    if (!frisk_fasta::read_index(index_path, f, idx, msg)) return fail(c, FRISK_E_INDEX, msg);
    std::vector<int64_t> lens(idx.size());
    std::vector<std::string> names(idx.size());
    for (size_t s = 0; s < idx.size(); ++s) { lens[s] = idx[s].len; names[s] = idx[s].name; }
    HIPC(c, hipSetDevice(c->device));
    if (int rc = plan_tiled_batch(c, lens, w, inc, flags, rank, world)) return rc;
    frisk_ctx::Batch& B = c->b();
    // the batch as it will sit on the device, assembled on the host from the mapping (PAD between the tiles), one upload
    frisk_fasta::ByteVec host;
    host.resize(size_t(B.padded_len));
    const int threads = host_threads(32, world);
    int64_t pos = 0;
    for (size_t t = 0; t < B.tiles.size(); ++t) {
        const int64_t off = B.seq_off[t], tlen = B.seq_len[t];
        std::memset(host.data() + pos, FRISK_PAD_BYTE, size_t(off - pos));
        if (tlen > 0) frisk_fasta::read_range_mt(f, idx[size_t(B.tiles[t].scaf)], B.tiles[t].base0, tlen, host.data() + off, threads);
        pos = off + (tlen > 0 ? tlen : 0);
    }
    std::memset(host.data() + pos, FRISK_PAD_BYTE, size_t(B.padded_len - pos));
    HIPC(c, B.d_ascii.reserve(size_t(B.padded_len)));
    if (int rc = h2d(c, B.d_ascii.p, host.data(), size_t(B.padded_len), c->stream)) return rc;
    HIPC(c, hipStreamSynchronize(c->stream));          // (the host copy goes away with this call)
    return finish_tiled(c, names, lens, n_seq_out, total_len_out, cand_begin, cand_end);
}

int32_t frisk_seq_count(const frisk_ctx* c) {
    if (!c || !c->b().have_seq) return 0;
    return c->b().tiled ? int32_t(c->b().g_len.size()) : c->b().n_seq;
}
const char* frisk_seq_name(const frisk_ctx* c, int32_t s) {
    if (!c || !c->b().have_seq || s < 0) return "";
    if (c->b().tiled) return size_t(s) < c->b().g_name.size() ? c->b().g_name[size_t(s)].c_str() : "";
    return s < c->b().n_seq ? c->b().seq_name[size_t(s)].c_str() : "";
}
int64_t frisk_seq_len(const frisk_ctx* c, int32_t s) {
    if (!c || !c->b().have_seq || s < 0) return -1;
    if (c->b().tiled) return size_t(s) < c->b().g_len.size() ? c->b().g_len[size_t(s)] : -1;
    return s < c->b().n_seq ? c->b().seq_len[size_t(s)] : -1;
}

// ---- double-buffered residency: upload the NEXT batch while the resident one is being profiled / scanned ----------
int frisk_seq_stage(frisk_ctx* c, const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq) {
    if (!c) return FRISK_E_ARG;
    if (n_seq > 0 && (!seqs || !lens)) return fail(c, FRISK_E_ARG, "null sequence table");
    frisk_ctx::Batch* B = nullptr;
    if (int rc = begin_stage(c, lens, n_seq, B)) return rc;
    if (int rc = enqueue_ascii_upload(c, *B, seqs, lens, n_seq, c->copy_stream)) return rc;
    if (int rc = alloc_packed(c, B, c->copy_stream)) return rc;
    if (int rc = enqueue_pack(c, *B, c->copy_stream)) return rc;
    return end_stage(c, *B);
}

int frisk_seq_stage_packed(frisk_ctx* c, const uint32_t* codes, const uint32_t* inv, const uint32_t* low, const int64_t* lens,
                           int32_t n_seq) {
    if (!c) return FRISK_E_ARG;
    if (!codes || !inv || !low || (n_seq > 0 && !lens)) return fail(c, FRISK_E_ARG, "null packed arrays");
    frisk_ctx::Batch* B = nullptr;
    if (int rc = begin_stage(c, lens, n_seq, B)) return rc;
    if (int rc = alloc_packed(c, B, c->copy_stream)) return rc;
    const size_t w32 = size_t(B->padded_len / 32);
    // (h2d: page-locked sources asynchronously; pageable ones - the memory-mapped sequence cache - through the context's
    //  page-locked pieces at PCIe rate instead of the runtime's own staging)
    if (int rc = h2d(c, B->d_codes.p, codes, 2 * w32 * 4, c->copy_stream)) return rc;
    if (int rc = h2d(c, B->d_inv.p, inv, w32 * 4, c->copy_stream)) return rc;
    if (int rc = h2d(c, B->d_low.p, low, w32 * 4, c->copy_stream)) return rc;
    return end_stage(c, *B);
}

// ---- the 0.25 B/base upload form: 2-bit codes densely, the two masks as run lists, the codes in pieces --------------------
int64_t frisk_padded_len_of(const int64_t* lens, int32_t n_seq) {
    if (n_seq < 0 || (n_seq > 0 && !lens)) return -1;
    for (int32_t s = 0; s < n_seq; ++s) if (lens[s] < 0) return -1;
    return frisk_pack2::padded_len(lens, n_seq);
}

int frisk_pack_2bit(const uint8_t* const* seqs, const int64_t* lens, int32_t n_seq, uint32_t* codes, int64_t** inv_runs,
                    int64_t* n_inv, int64_t** low_runs, int64_t* n_low) {
    if (n_seq < 0 || (n_seq > 0 && (!seqs || !lens)) || !codes || !inv_runs || !n_inv || !low_runs || !n_low) return FRISK_E_ARG;
    for (int32_t s = 0; s < n_seq; ++s) if (lens[s] < 0 || (lens[s] > 0 && !seqs[s])) return FRISK_E_ARG;
    frisk_pack2::Runs R;
    frisk_pack2::pack_batch(seqs, lens, n_seq, codes, R, host_threads(32));
    return give_runs(R.inv, R.low, inv_runs, n_inv, low_runs, n_low) ? FRISK_OK : FRISK_E_HIP;
}

int frisk_fasta_load(frisk_ctx* c, const char* path, int32_t* n_seq_out, int64_t* total_len_out) {
    if (!c || !path) return FRISK_E_ARG;
    frisk_fasta::Records rec;
    std::string err;
#ifdef FRISK_TUNE
    const auto tt0 = std::chrono::steady_clock::now();
#endif
    // Read and packed on the HOST, by the reader's threads, straight into the 0.25 B/base form (fasta_pack2.h: no one-byte-per-base
    // buffer in between; seq_pack2.h: 2-bit codes + run lists of the two masks).  PCIe then carries a quarter of the bytes (3.3 GB
    // of ASCII -> 0.82 GB for a GRCh38-sized assembly), and the host copy stays until the next load: the CLI's sequence cache is
    // written from it without touching the device.
    frisk_fasta::CodeVec packed;
    frisk_pack2::Runs packed_runs;
    if (!frisk_fasta::parse_pack(path, rec, packed, packed_runs, err, host_threads(32))) return fail(c, FRISK_E_ARG, err);
#ifdef FRISK_TUNE
    const auto tt1 = std::chrono::steady_clock::now();
#endif
    HIPC(c, hipSetDevice(c->device));
    int rc = layout_batch(c, rec.lens.data(), int32_t(rec.lens.size()));
    if (rc) return rc;
    frisk_ctx::Batch& B = c->b();
    B.seq_name = rec.names;
    if (packed.size() != size_t(B.padded_len / 32) * 2) return fail(c, FRISK_E_STATE, "frisk_fasta_load: packed length and batch layout disagree");
    B.h_codes.swap(packed);
    B.h_runs = std::move(packed_runs);
    B.have_host2 = true;
#ifdef FRISK_TUNE
    const auto tt2 = std::chrono::steady_clock::now();
#endif
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    rc = upload_2bit(c, B, B.h_codes.data(), B.h_runs.inv.data(), int64_t(B.h_runs.inv.size() / 2), B.h_runs.low.data(),
                     int64_t(B.h_runs.low.size() / 2), 0, c->stream);
    if (rc) return rc;
    rc = finish_timed_load(c);                  // (upload + mask expansion: there is no device-side packing on this path)
    if (rc) return rc;
#ifdef FRISK_TUNE
    {
        const auto tt3 = std::chrono::steady_clock::now();
        auto msf = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        if (std::getenv("FRISK_LOAD_SPLIT")) std::fprintf(stderr, "[load] read + pack %.1f ms, layout %.1f ms, upload %.1f ms\n", msf(tt0, tt1), msf(tt1, tt2), msf(tt2, tt3));
    }
#endif
    int64_t total = 0;
    for (int64_t v : rec.lens) total += v;
    if (n_seq_out) *n_seq_out = int32_t(rec.lens.size());
    if (total_len_out) *total_len_out = total;
    return FRISK_OK;
}

int frisk_seq_stage_2bit(frisk_ctx* c, const uint32_t* codes, const int64_t* inv_runs, int64_t n_inv, const int64_t* low_runs,
                         int64_t n_low, const int64_t* lens, int32_t n_seq, int64_t piece_bases) {
    if (!c) return FRISK_E_ARG;
    if (!codes || (n_seq > 0 && !lens) || (n_inv != 0 && !inv_runs) || (n_low != 0 && !low_runs))
        return fail(c, FRISK_E_ARG, "frisk_seq_stage_2bit: null array");
    if (piece_bases < 0) return fail(c, FRISK_E_ARG, "frisk_seq_stage_2bit: piece_bases < 0");
    frisk_ctx::Batch* B = nullptr;
    if (int rc = begin_stage(c, lens, n_seq, B)) return rc;
    if (int rc = upload_2bit(c, *B, codes, inv_runs, n_inv, low_runs, n_low, piece_bases, c->copy_stream)) return rc;
    return end_stage(c, *B, true);
}

int frisk_seq_commit(frisk_ctx* c) {
    if (!c) return FRISK_E_ARG;
    if (!c->staged) return fail(c, FRISK_E_STATE, "frisk_seq_commit: no staged batch");
    HIPC(c, hipSetDevice(c->device));
    // the slot that stops being resident here is the one the next stage fills: that upload waits for what is queued so far
    HIPC(c, hipEventRecord(c->slot_free_ev, c->stream));
    c->slot_ev_set = true;
    // the compute stream waits on the device; the host does not.  A streamed batch is waited for piece by piece, by its first user
    if (!c->bat[c->cur ^ 1].streaming) HIPC(c, hipStreamWaitEvent(c->stream, c->staged_ev, 0));
    c->cur ^= 1;
    c->b().have_seq = true;
    c->staged = false;
    c->plan_w = -1;
    return FRISK_OK;
}

int frisk_seq_export_2bit(frisk_ctx* c, uint32_t* codes, int64_t** inv_runs, int64_t* n_inv, int64_t** low_runs, int64_t* n_low) {
    if (!c || !codes || !inv_runs || !n_inv || !low_runs || !n_low) return FRISK_E_ARG;
    if (!c->b().have_seq) return fail(c, FRISK_E_STATE, "no resident sequence batch");
    const frisk_ctx::Batch& B = c->b();
    if (B.have_host2) {                 // packed on the host by frisk_fasta_load: the device is not involved
        const size_t nbytes = B.h_codes.size() * 4;
        const int T = int(std::max<size_t>(1, std::min<size_t>(8, nbytes >> 26)));
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) {
            const size_t a = nbytes / 64 * size_t(t) / size_t(T) * 64, b = t + 1 == T ? nbytes : nbytes / 64 * size_t(t + 1) / size_t(T) * 64;
            th.emplace_back([&, a, b] { std::memcpy(reinterpret_cast<char*>(codes) + a, reinterpret_cast<const char*>(B.h_codes.data()) + a, b - a); });
        }
        for (auto& x : th) x.join();
        if (!give_runs(B.h_runs.inv, B.h_runs.low, inv_runs, n_inv, low_runs, n_low)) return fail(c, FRISK_E_HIP, "out of host memory");
        return FRISK_OK;
    }
    HIPC(c, hipSetDevice(c->device));
    if (int rc = settle_stream(c)) return rc;
    std::vector<uint32_t> inv(size_t(B.padded_len / 32)), low(size_t(B.padded_len / 32));
    if (int rc = d2h_packed(c, codes, inv.data(), low.data())) return rc;
    std::vector<int64_t> ri, rl;
    std::thread t([&] { frisk_pack2::bitmap_runs(inv.data(), B.seq_len.data(), B.n_seq, ri); });
    frisk_pack2::bitmap_runs(low.data(), B.seq_len.data(), B.n_seq, rl);
    t.join();
    if (!give_runs(ri, rl, inv_runs, n_inv, low_runs, n_low)) return fail(c, FRISK_E_HIP, "out of host memory");
    return FRISK_OK;
}

int frisk_seq_export_packed(frisk_ctx* c, uint32_t* codes, uint32_t* inv, uint32_t* low) {
    if (!c || !codes || !inv || !low) return FRISK_E_ARG;
    if (!c->b().have_seq) return fail(c, FRISK_E_STATE, "no resident sequence batch");
    HIPC(c, hipSetDevice(c->device));
    if (int rc = settle_stream(c)) return rc;
    return d2h_packed(c, codes, inv, low);
}

int frisk_seq_set_names(frisk_ctx* c, const char* const* names, int32_t n_seq) {
    if (!c || (n_seq > 0 && !names)) return FRISK_E_ARG;
    if (!c->b().have_seq || n_seq != c->b().n_seq) return fail(c, FRISK_E_ARG, "frisk_seq_set_names: one name per resident scaffold");
    for (int32_t s = 0; s < n_seq; ++s) c->b().seq_name[size_t(s)] = names[s] ? names[s] : "";
    return FRISK_OK;
}

int frisk_seq_synth(frisk_ctx* c, const int64_t* lens, int32_t n_seq, uint64_t seed, double island_frac,
                    double n_frac, double lower_frac, double repeats_per_kb) {
    return frisk_seq_synth2(c, lens, n_seq, seed, island_frac, n_frac, lower_frac, repeats_per_kb, 0.0, 0.0);
}

int frisk_seq_synth2(frisk_ctx* c, const int64_t* lens, int32_t n_seq, uint64_t seed, double island_frac,
                     double n_frac, double lower_frac, double repeats_per_kb, double period_mix, double sat_frac) {
    if (!c) return FRISK_E_ARG;
    if (n_seq > 0 && !lens) return fail(c, FRISK_E_ARG, "null length table");
    HIPC(c, hipSetDevice(c->device));
    int rc = layout_batch(c, lens, n_seq);
    if (rc) return rc;
    HIPC(c, c->b().d_ascii.reserve(size_t(c->b().padded_len)));
    HIPC(c, hipMemsetAsync(c->b().d_ascii.p, FRISK_PAD_BYTE, size_t(c->b().padded_len), c->stream));
    SynthTables tabs;
    synth_make_tables(seed, tabs);
    const uint32_t thr_island = synth_frac_to_u32(island_frac), thr_nbig = synth_frac_to_u32(n_frac * 0.8),
                   thr_nsmall = synth_frac_to_u32(n_frac * 0.2), thr_low = synth_frac_to_u32(lower_frac),
                   thr_rep = synth_frac_to_u32(repeats_per_kb * (SYNTH_REP / 1000.0)), thr_mix = synth_frac_to_u32(period_mix),
                   thr_sat = synth_frac_to_u32(sat_frac * (2.0 * SYNTH_SAT_GROUP / (SYNTH_SAT_GROUP + 1.0))),
                   thr_div = synth_frac_to_u32(SYNTH_SAT_DIV);
    for (int32_t s = 0; s < n_seq; ++s) {
        if (lens[s] <= 0) continue;
        const int64_t nblk = (lens[s] + SYNTH_BLOCK - 1) / SYNTH_BLOCK;
        synth_kernel<<<grid_for(nblk, 64, 1 << 20), 64, 0, c->stream>>>(c->b().d_ascii.p + c->b().seq_off[size_t(s)], lens[s],
                                                                       seed, uint32_t(s), tabs, thr_island, thr_nbig,
                                                                       thr_nsmall, thr_low, thr_rep, thr_mix, thr_sat, thr_div);
        HIPC(c, hipGetLastError());
    }
    rc = alloc_packed(c);
    if (rc) return rc;
    return run_pack(c);
}

// A batch of null sequences drawn from the order-`order` Markov chain of the finalised profile (null_kernels.h): laid out, packed
// and made resident as frisk_seq_synth2 does it.  The profile is only read.
int frisk_seq_null(frisk_ctx* c, const int64_t* lens, int32_t n_seq, uint64_t seed, int32_t order) {
    if (!c) return FRISK_E_ARG;
    if (n_seq < 0) return fail(c, FRISK_E_ARG, "n_seq < 0");
    if (n_seq > 0 && !lens) return fail(c, FRISK_E_ARG, "null length table");
    if (order < 0 || order + 1 < c->kmin || order + 1 > c->kmax)
        return fail(c, FRISK_E_ARG, "frisk_seq_null: the chain of order r reads the counts of order r + 1, which must lie in kmin .. kmax");
    std::vector<int64_t> meta(3 * size_t(n_seq) + 1);         // blk0 [n_seq + 1], then off and len [n_seq] each (off: filled below)
    int64_t blocks = 0, bases = 0;
    for (int32_t s = 0; s < n_seq; ++s) {
        if (lens[s] < 0) return fail(c, FRISK_E_ARG, "negative scaffold length");
        if (lens[s] >= INT64_MAX - 64 - bases) return fail(c, FRISK_E_ARG, "frisk_seq_null: the batch's length does not fit 63 bits");
        bases += lens[s] + 1;
        meta[size_t(s)] = blocks;
        blocks += (lens[s] + NULL_BLOCK - 1) / NULL_BLOCK;
    }
    meta[size_t(n_seq)] = blocks;
    if (!c->profile_final) return fail(c, FRISK_E_STATE, "frisk_seq_null: no finalised profile");
    HIPC(c, hipSetDevice(c->device));
    if (!c->evn0) {
        HIPC(c, hipEventCreate(&c->evn0));
        HIPC(c, hipEventCreate(&c->evn1));
    }
    int rc = layout_batch(c, lens, n_seq);
    if (rc) return rc;
    frisk_ctx::Batch& B = c->b();
    HIPC(c, B.d_ascii.reserve(size_t(B.padded_len)));
    HIPC(c, hipMemsetAsync(B.d_ascii.p, FRISK_PAD_BYTE, size_t(B.padded_len), c->stream));
    const int64_t n_ctx = int64_t(1) << (2 * order);
    DevBuf<uint64_t> d_cum;             // (both freed on every return below; run_pack waits for the kernels that read them)
    DevBuf<int64_t> d_meta;
    HIPC(c, d_cum.reserve(size_t(4 * n_ctx), size_t(4 * n_ctx)));
    HIPC(c, d_meta.reserve(meta.size(), meta.size()));
    for (int32_t s = 0; s < n_seq; ++s) {
        meta[size_t(n_seq) + 1 + size_t(s)] = B.seq_off[size_t(s)];
        meta[2 * size_t(n_seq) + 1 + size_t(s)] = lens[s];
    }
    HIPC(c, hipMemcpyAsync(d_meta.p, meta.data(), meta.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipEventRecord(c->evn0, c->stream));
    null_table_kernel<<<grid_for(n_ctx, 256, c->num_cu * 8), 256, 0, c->stream>>>(c->d_sym.p + table_offset(c->kmin, order + 1), n_ctx, d_cum.p);
    HIPC(c, hipGetLastError());
    if (blocks > 0) {
        null_kernel<<<grid_for(blocks, 64, 1 << 20), 64, 0, c->stream>>>(B.d_ascii.p, d_meta.p, d_meta.p + n_seq + 1, d_meta.p + 2 * size_t(n_seq) + 1,
                                                                        n_seq, d_cum.p, uint32_t(n_ctx - 1), seed);
        HIPC(c, hipGetLastError());
    }
    HIPC(c, hipEventRecord(c->evn1, c->stream));
    rc = alloc_packed(c);
    if (rc) return rc;
    rc = run_pack(c);
    if (rc) return rc;
    float ms = 0;
    HIPC(c, hipEventElapsedTime(&ms, c->evn0, c->evn1));
    c->ms[6] = ms;
    return FRISK_OK;
}

int frisk_seq_read(frisk_ctx* c, int32_t s, int64_t offset, int64_t n, uint8_t* out) {
    if (!c || !out) return FRISK_E_ARG;
    if (!c->b().have_seq) return fail(c, FRISK_E_STATE, "no resident sequence batch");
    if (c->b().tiled) return fail(c, FRISK_E_STATE, "frisk_seq_read: the resident batch holds tiles, not whole scaffolds");
    if (s < 0 || s >= c->b().n_seq) return fail(c, FRISK_E_ARG, "sequence index out of range");
    if (offset < 0 || n < 0 || offset + n > c->b().seq_len[size_t(s)]) return fail(c, FRISK_E_ARG, "range outside the scaffold");
    if (n == 0) return FRISK_OK;
    HIPC(c, hipSetDevice(c->device));
    if (int rs = settle_stream(c)) return rs;
    DevBuf<uint8_t> tmp;            // (freed on every return below)
    HIPC(c, tmp.reserve(size_t(n)));
    unpack_kernel<<<grid_for(n, 256, c->num_cu * 8), 256, 0, c->stream>>>(c->b().d_codes.p, c->b().d_inv.p, c->b().d_low.p,
                                                                           c->b().seq_off[size_t(s)] + offset, n, tmp.p);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, tmp.p, size_t(n), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return FRISK_OK;
}

}  // extern "C"
