// profile_plan.h - everything the host decides about phase A (frisk_profile_add) before it touches the device, as plain values
// computed by pure functions: which of the three kernels of profile_kernels.h counts a range of positions and on what grid
// (plan_profile_launch), and the ranges in which a streamed batch is counted behind its upload (plan_profile_pieces).  No HIP here:
// frisk_abi.hip fills the arguments from the context and launches the plan; tools/exp/san_host.cpp computes and checks plans on a CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/frisk_hip.h"      // FRISK_PROFILE_ONE_PASS, the caller's flag (found without an include path of its own)

// K = 8, a long range (a whole resident genome): 16-bit counters, ONE walk over the sequence (profile_add16_kernel; a wrapped
// counter sends its workgroup to the two-half form).  The walk halves, the flush doubles (65 536 fields per workgroup instead of
// 32 768 bins): measured 2.42 -> 1.33 ms on the 3.29 Gb shape, 0.345 -> 0.55 ms on the 410 Mb shard (tools/exp/prof_ab.py) - so from
// 2^30 positions per launch on.  (FRISK_PROFILE_ONE_PASS forces it: the tests' way to the overflow path.)
constexpr int64_t PROFILE_ONE_PASS_MIN = int64_t(1) << 30;
// a workgroup of the forms with a table in LDS is worth its table's flush from this many positions on: no more chunks than that
constexpr int64_t PROFILE_CHUNK_POSITIONS = 65536;
// measured on the 410 Mb shard: 1 -> 0.34 ms, 2 -> 0.41, 4 -> 0.51 (the flush of the private tables dominates)
constexpr int64_t PROFILE_WG_PER_CU = 1;
constexpr int PROFILE_LDS_THREADS = 1024;   // = FRISK_PROF_NT, a lane a bitmap word
constexpr int PROFILE_BIG_THREADS = 256, PROFILE_BIG_WG_PER_CU = 8;

enum ProfileForm {
    PROFILE_FORM_BIG,       // kmax > 8: 4^K counters do not fit a CU, one global atomic per position (profile_add_big_kernel)
    PROFILE_FORM_ONE_PASS,  // kmax = 8, long or forced: 16-bit fields in LDS, one walk (profile_add16_kernel)
    PROFILE_FORM_LDS        // order-K table privatised in LDS as 32-bit counters, in two halves at K = 8 where 256 KiB do not fit a
};                          // CU (profile_add_kernel)

struct ProfileLaunch {
    ProfileForm form = PROFILE_FORM_LDS;
    int grid = 0;               // 0: an empty range, nothing to launch
    int threads = 0;
    size_t lds_bytes = 0;       // dynamic LDS
    int halves = 1;             // workgroups per chunk (2: each walks the chunk for its half of the k-mer space)
    int64_t chunk_words = 0;    // bitmap words of a chunk (0 in the big form: a grid-stride loop)
    int64_t nwords = 0;         // bitmap words that hold [p0, p1): a lane takes one
};

// num_cu: the device's; [p0, p1): padded positions, p0 <= p1; one_pass: FRISK_PROFILE_ONE_PASS
inline ProfileLaunch plan_profile_launch(int kmax, int num_cu, int64_t p0, int64_t p1, bool one_pass) {
    ProfileLaunch L;
    const int64_t span = p1 - p0;
    L.nwords = span > 0 ? ((p1 + 31) >> 5) - (p0 >> 5) : 0;
    if (kmax > 8) {
        L.form = PROFILE_FORM_BIG;
        L.threads = PROFILE_BIG_THREADS;
        const int64_t blocks = (L.nwords + PROFILE_BIG_THREADS - 1) / PROFILE_BIG_THREADS;
        L.grid = int(std::min<int64_t>(blocks, int64_t(num_cu) * PROFILE_BIG_WG_PER_CU));
        return L;
    }
    const bool one = kmax == 8 && (one_pass || span >= PROFILE_ONE_PASS_MIN);
    L.form = one ? PROFILE_FORM_ONE_PASS : PROFILE_FORM_LDS;
    L.threads = PROFILE_LDS_THREADS;
    L.halves = (kmax == 8 && !one) ? 2 : 1;
    // 4^8 16-bit fields, or the 32-bit counters of one half (K = 1: 16 bytes, and never less: the kernel clears by 16-byte stores)
    L.lds_bytes = one ? size_t(131072) : std::max<size_t>((size_t(1) << (2 * kmax)) / size_t(L.halves) * 4, 16);
    // (a single CU holds no two halves beside each other: one chunk all the same)
    const int64_t max_chunks = std::max<int64_t>(1, int64_t(num_cu) * PROFILE_WG_PER_CU / L.halves);
    int64_t nchunks = std::min<int64_t>(std::max<int64_t>(1, span / PROFILE_CHUNK_POSITIONS), max_chunks);
    L.chunk_words = (L.nwords + nchunks - 1) / nchunks;
    nchunks = L.chunk_words > 0 ? (L.nwords + L.chunk_words - 1) / L.chunk_words : 0;     // (no chunk without a word)
    L.grid = int(nchunks) * L.halves;
    return L;
}

// A streamed batch (frisk_seq_stage_2bit) counted as a whole: phase A follows the copies piece by piece - the kernel of piece i runs
// while piece i + 1 crosses PCIe, only the last piece's kernel is left when the upload ends.  piece_end[i]: the bitmap word behind
// piece i.  A lane that counts the positions of bitmap word q reads word q + 1 of the masks and code word 2 q + 2, so piece i's
// kernel stops one word short of its end.  The first piece always launches (the start event is recorded with it) and the last
// always (the end event; it runs to padded_len), even where they add no position; the others only where they add some.
struct ProfilePiece {
    int64_t p0, p1;         // positions to count once the pieces 0 .. piece have arrived
    bool first, last;
    size_t piece;
};

inline std::vector<ProfilePiece> plan_profile_pieces(const std::vector<int64_t>& piece_end, int64_t padded_len) {
    std::vector<ProfilePiece> out;
    const size_t np = piece_end.size();
    int64_t done = 0;
    for (size_t i = 0; i < np; ++i) {
        const bool first = i == 0, last = i + 1 == np;
        const int64_t upto = std::max(done, last ? padded_len : (piece_end[i] - 1) * 32);
        if (upto > done || first || last) out.push_back(ProfilePiece{done, upto, first, last, i});
        done = upto;
    }
    return out;
}
