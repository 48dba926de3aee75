// panel_kernels.h - frisk_score_ranges_panel: the rows of range_kernels.h against a PANEL of genome-side tables in one pass.  A
// range is counted once - stages 1 and 2 are range_kernels.h's own (range_short_tables, range_long_tables) - and only stages
// 3 + 4 are new: what a present max-mer takes from the range (W, A: eight prefix counts, the orphan lookup) is computed once, what
// it takes from a profile (one genome-side value, a product, div_exact, log_pos, three exact additions) once per profile.
//
// Layout of the panel: tiles of FRISK_PANEL_TILE profiles, a tile = [code][FRISK_PANEL_TILE] doubles, so the values a lane needs
// for one max-mer are 64 contiguous bytes.  A tile's unused slots hold 1.0 (never NaN); their sums are not written.  A panel of
// more than one tile walks the range's order-K table once per tile.
//
// Short form (the geometry of range_short_kernel): the walk does not score.  A wave appends the codes of its share's non-empty bins
// to a wave-private list in LDS - the position from ballots over the lanes, 16-bit codes - and whenever the list holds 64 or more
// it scores 64 of them, one per lane, with every lane busy; the rest is flushed behind the walk.  (range_short_kernel scores inside
// the walk: at K = 8 the FP64 body runs 128 times per range with a twelfth of its lanes active.)  No workgroup barrier inside the
// walk.  Long form (range_long_kernel's): the profile loop over cnt[offK + code] != 0, FRISK_PANEL_TILE_LONG profiles at a time -
// 1024 threads leave a lane 128 registers, and a profile's three ExactSums take 12.
//
// Why plane p is bit for bit the single-profile row: ExactSum totals do not depend on which lane scored which max-mer
// (scan_kernel.h, at FRISK_EXACT_BIAS), and every other operation on a max-mer is range_score_maxmer's, in its order
// (range_maxmer_window, range_maxmer_add); the reduction and the KLD are range_finish itself.
//
// FP64 throughout, no MFMA, no floating-point atomics.
#pragma once
#include "frisk_hip.h"
#include "range_kernels.h"

#pragma clang fp contract(off)

#define FRISK_PANEL_TILE_LONG 2     // long form: profiles scored per walk (a divisor of FRISK_PANEL_TILE)
#define FRISK_PANEL_LIST (512 + 64) // short form: entries of a wave's list - under 64 left over, at most 8 bins x 64 lanes appended
#define FRISK_PANEL_TILES (FRISK_PANEL_MAX / FRISK_PANEL_TILE)

static_assert(FRISK_PANEL_MAX % FRISK_PANEL_TILE == 0 && FRISK_PANEL_TILE % FRISK_PANEL_TILE_LONG == 0, "whole tiles");

struct PanelParams {
    RangeParams R;                              // R.ig is not used; R.status and R.kld are plane 0
    const double* tile[FRISK_PANEL_TILES];      // [code][FRISK_PANEL_TILE] each
    int32_t n_prof;                             // profiles in the panel, >= 1
    int64_t plane;                              // rows per plane of status / kld
};

// LDS of the short form: range_lds, then the waves' lists
__host__ __device__ inline uint32_t panel_lds_list(int kmin, int kmax) { return (range_lds(kmin, kmax).total + 15u) / 16u * 16u; }
__host__ __device__ inline uint32_t panel_lds_total(int kmin, int kmax) {
    return panel_lds_list(kmin, kmax) + (FRISK_RANGE_NT / 64) * FRISK_PANEL_LIST * 2;
}

// frisk_panel_push: ig -> slot `slot` of a tile; `fresh`: the tile is new, its other slots become 1.0
__global__ void panel_store_kernel(const double* __restrict__ ig, double* __restrict__ tile, int64_t n, int slot, int fresh) {
    for (int64_t c = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; c < n; c += int64_t(gridDim.x) * blockDim.x) {
        if (fresh) for (int j = 0; j < FRISK_PANEL_TILE; ++j) tile[c * FRISK_PANEL_TILE + j] = 1.0;
        tile[c * FRISK_PANEL_TILE + slot] = ig[c];
    }
}

// a row the N rule drops: range_write_unresolved has written plane 0 and the shared columns; one thread
__device__ inline void panel_write_unresolved(const PanelParams& Q, int64_t row) {
    for (int p = 1; p < Q.n_prof; ++p) {
        Q.R.status[p * Q.plane + row] = 0u;
        Q.R.kld[p * Q.plane + row] = __longlong_as_double(0x7FF8000000000000LL);
    }
}

// the list's stores and loads are ordered within the wave: LDS serves a wave's operations in order, the compiler must keep them so
__device__ inline void panel_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- short form -------------------------------------------------------------------------------------------------------------
template <bool K8>
__global__ __launch_bounds__(FRISK_RANGE_NT) void panel_short_kernel(const PanelParams Q) {
    constexpr int NT = FRISK_RANGE_NT, NW = NT / 64, TP = FRISK_PANEL_TILE;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t tl[8];
    __shared__ double red[TP * NW * 6];         // one slice per profile of the tile: its reductions need no barrier between them
    const RangeParams& P = Q.R;
    const int tid = threadIdx.x, lane = tid & 63;
    const int kmin = P.kmin;
    const int kmax = K8 ? 8 : P.kmax;
    const RangeLds L = range_lds(kmin, kmax);
    const uint32_t* t8 = reinterpret_cast<const uint32_t*>(lds);
    const uint16_t* small16 = reinterpret_cast<const uint16_t*>(lds + L.small);
    uint16_t* mylist = reinterpret_cast<uint16_t*>(lds + panel_lds_list(kmin, kmax)) + (tid >> 6) * FRISK_PANEL_LIST;
    const uint32_t nK = 1u << (2 * kmax);
    const uint32_t offK = K8 ? 0u : uint32_t(table_offset(kmin, kmax));

    const int64_t n_rows = range_rows(P);
    for (int64_t q = blockIdx.x; q < n_rows; q += gridDim.x) {
        const int64_t row = P.list[q];
        WinTables<K8> T;
        int64_t S;
        uint32_t nvalid_top;
        const int what = range_short_tables<K8>(P, row, lds, tl, T, S, nvalid_top);
        if (what == RANGE_ROW_DROPPED && tid == 0) panel_write_unresolved(Q, row);
        if (what != RANGE_ROW_SCORE) continue;
        auto count = [&](int x, uint32_t c) -> uint32_t { return T.count(x, c); };
        const uint32_t status = range_status(nvalid_top, S, kmin, kmax);
        double r[FRISK_MAX_K + 1];
        range_constants(S, r);

        for (int t0 = 0; t0 < Q.n_prof; t0 += TP) {
            const double* __restrict__ g = Q.tile[t0 / TP];
            ExactSum accw[TP], accg[TP], acct[TP];
#pragma unroll
            for (int j = 0; j < TP; ++j) accw[j] = accg[j] = acct[j] = exact_begin();
            // one listed max-mer per lane, densely: W and A once, then the tile's profiles
            auto score = [&](uint32_t code) {
                unsigned long long W;
                double A;
                range_maxmer_window(code, kmin, kmax, r, count, W, A);
                const double Wd = double(W);
                const double* gv = g + size_t(code) * TP;
#pragma unroll
                for (int j = 0; j < TP; ++j) range_maxmer_add(A, Wd, gv[j], accw[j], accg[j], acct[j]);
            };
            uint32_t nlist = 0;                 // wave-uniform: entries of the wave's list
            auto push = [&](bool present, uint32_t code) {
                const unsigned long long m = __ballot(present);
                const uint32_t before = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
                if (present) mylist[nlist + before] = uint16_t(code);
                nlist += uint32_t(__popcll(m));
            };
            auto drain = [&]() {                // full waves only
                panel_wave_order();
                while (nlist >= 64u) {
                    nlist -= 64u;
                    score(mylist[nlist + lane]);
                }
                panel_wave_order();
            };
            if (K8) {
                for (uint32_t base = 0; base < nK / 8; base += NT) {        // eight bins per lane and step: at most 512 new entries
                    const uint32_t grp = base + tid;
                    const uint4 v = reinterpret_cast<const uint4*>(t8)[grp];
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int b = 0; b < 8; ++b) push(((w[b >> 1] >> ((b & 1) * 16)) & 0xFFFFu) != 0u, 8 * grp + b);
                    drain();
                }
            } else {
                for (uint32_t base = 0; base < nK; base += NT) {            // one bin per lane and step
                    const uint32_t code = base + tid;
                    push(code < nK && small16[offK + (code < nK ? code : 0u)] != 0, code);
                    drain();
                }
            }
            if (uint32_t(lane) < nlist) score(mylist[lane]);                // the remainder, under 64
            panel_wave_order();
#pragma unroll
            for (int j = 0; j < TP; ++j)
                if (t0 + j < Q.n_prof)
                    range_finish<NW>(P, (t0 + j) * Q.plane + row, status, nvalid_top, accw[j], accg[j], acct[j], red + j * NW * 6);
        }
    }
}

// ---- long form --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FRISK_RANGE_BIG_NT) void panel_long_kernel(const PanelParams Q, uint32_t* __restrict__ big, int64_t big_stride) {
    constexpr int NT = FRISK_RANGE_BIG_NT, NW = NT / 64, TP = FRISK_PANEL_TILE, TL = FRISK_PANEL_TILE_LONG;
    __shared__ uint32_t tl[8];
    __shared__ double red[TL * NW * 6];
    const RangeParams& P = Q.R;
    const int tid = threadIdx.x;
    const int kmin = P.kmin, kmax = P.kmax;
    uint32_t* cnt = big + int64_t(blockIdx.x) * big_stride;
    const int64_t offK = table_offset(kmin, kmax);
    const uint32_t nK = 1u << (2 * kmax);
    const int64_t n_rows = range_rows(P);
    for (int64_t q = blockIdx.x; q < n_rows; q += gridDim.x) {
        const int64_t row = P.list[q];
        int64_t S;
        uint32_t nvalid_top;
        const int what = range_long_tables(P, row, cnt, big_stride, tl, S, nvalid_top);
        if (what == RANGE_ROW_DROPPED && tid == 0) panel_write_unresolved(Q, row);
        if (what != RANGE_ROW_SCORE) continue;
        auto count = [&](int x, uint32_t c) -> uint32_t { return cnt[table_offset(kmin, x) + c]; };
        const uint32_t status = range_status(nvalid_top, S, kmin, kmax);
        double r[FRISK_MAX_K + 1];
        range_constants(S, r);
        for (int t0 = 0; t0 < Q.n_prof; t0 += TL) {
            const double* __restrict__ g = Q.tile[t0 / TP] + (t0 % TP);
            ExactSum accw[TL], accg[TL], acct[TL];
#pragma unroll
            for (int j = 0; j < TL; ++j) accw[j] = accg[j] = acct[j] = exact_begin();
            for (uint32_t code = tid; code < nK; code += NT) {
                if (cnt[offK + code] == 0) continue;
                unsigned long long W;
                double A;
                range_maxmer_window(code, kmin, kmax, r, count, W, A);
                const double Wd = double(W);
                const double* gv = g + size_t(code) * TP;
#pragma unroll
                for (int j = 0; j < TL; ++j) range_maxmer_add(A, Wd, gv[j], accw[j], accg[j], acct[j]);
            }
#pragma unroll
            for (int j = 0; j < TL; ++j)
                if (t0 + j < Q.n_prof)
                    range_finish<NW>(P, (t0 + j) * Q.plane + row, status, nvalid_top, accw[j], accg[j], acct[j], red + j * NW * 6);
        }
        range_zero_tables(cnt, big_stride);     // (behind range_finish's barrier: every read of the tables is done)
    }
}
