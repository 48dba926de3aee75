// panel_kernels.h - frisk_score_ranges_panel: the rows of range_kernels.h against a PANEL of genome-side tables in one pass.  A
// range is counted once - the forms and the row loop are range_kernels.h's own (ShortForm, LongForm, range_row_loop) - and only
// stages 3 + 4, the two modes here, are new: what a present max-mer takes from the range (W, A: eight prefix counts, the orphan
// lookup) is computed once, what it takes from a profile (one genome-side value, a product, div_exact, log_pos, three exact
// additions) once per profile.
//
// Layout of the panel: tiles of FRISK_PANEL_TILE profiles, a tile = [code][FRISK_PANEL_TILE] doubles, so the values a lane needs
// for one max-mer are 64 contiguous bytes.  A tile's unused slots hold 1.0 (never NaN); their sums are not written.  A panel of
// more than one tile walks the range's order-K table once per tile.
//
// Short form (PanelShortMode, the geometry of range_short_kernel): the walk does not score.  A wave appends the codes of its
// share's non-empty bins to a wave-private list in LDS - the position from ballots over the lanes, 16-bit codes - and whenever the
// list holds 64 or more it scores 64 of them, one per lane, with every lane busy; the rest is flushed behind the walk.  (PlainMode
// scores inside the walk: at K = 8 the FP64 body runs 128 times per range with a twelfth of its lanes active.)  No workgroup
// barrier inside the walk.  Long form (PanelLongMode): the profile loop inside the walk, FRISK_PANEL_TILE_LONG profiles at a time -
// 1024 threads leave a lane 128 registers, and a profile's three ExactSums take 12.  The short form holds a tile's 24 in 196 VGPRs.
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

// ---- the two scoring bodies -------------------------------------------------------------------------------------------------
// (modes of range_row_loop; `red`: one slice of NW * 6 doubles per profile scored together - their reductions need no barrier
// between them)
struct PanelShortMode {
    const PanelParams& Q;
    double* red;
    uint16_t* mylist;           // the wave's list
    __device__ void dropped(int64_t row) const { if (threadIdx.x == 0) panel_write_unresolved(Q, row); }
    template <bool K8>
    __device__ void score(const ShortForm<K8>& form, int64_t row, uint32_t status, uint32_t nvalid_top, const double* r) const {
        constexpr int NW = FRISK_RANGE_NT / 64, TP = FRISK_PANEL_TILE;
        const int lane = threadIdx.x & 63;
        const int kmin = form.kmin, kmax = form.kmax();
        auto count = [&](int x, uint32_t c) -> uint32_t { return form.count(x, c); };
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
            form.walk(push, drain);             // a step appends at most 8 bins x 64 lanes to under 64 left over
            if (uint32_t(lane) < nlist) score(mylist[lane]);                // the remainder, under 64
            panel_wave_order();
#pragma unroll
            for (int j = 0; j < TP; ++j)
                if (t0 + j < Q.n_prof)
                    range_finish<NW>(Q.R, (t0 + j) * Q.plane + row, status, nvalid_top, accw[j], accg[j], acct[j], red + j * NW * 6);
        }
    }
};

struct PanelLongMode {
    const PanelParams& Q;
    double* red;
    __device__ void dropped(int64_t row) const { if (threadIdx.x == 0) panel_write_unresolved(Q, row); }
    __device__ void score(const LongForm& form, int64_t row, uint32_t status, uint32_t nvalid_top, const double* r) const {
        constexpr int NW = FRISK_RANGE_BIG_NT / 64, TP = FRISK_PANEL_TILE, TL = FRISK_PANEL_TILE_LONG;
        const int kmin = form.kmin, kmax = form.kmax();
        auto count = [&](int x, uint32_t c) -> uint32_t { return form.count(x, c); };
        for (int t0 = 0; t0 < Q.n_prof; t0 += TL) {
            const double* __restrict__ g = Q.tile[t0 / TP] + (t0 % TP);
            ExactSum accw[TL], accg[TL], acct[TL];
#pragma unroll
            for (int j = 0; j < TL; ++j) accw[j] = accg[j] = acct[j] = exact_begin();
            form.walk([&](bool present, uint32_t code) {
                if (!present) return;
                unsigned long long W;
                double A;
                range_maxmer_window(code, kmin, kmax, r, count, W, A);
                const double Wd = double(W);
                const double* gv = g + size_t(code) * TP;
#pragma unroll
                for (int j = 0; j < TL; ++j) range_maxmer_add(A, Wd, gv[j], accw[j], accg[j], acct[j]);
            });
#pragma unroll
            for (int j = 0; j < TL; ++j)
                if (t0 + j < Q.n_prof)
                    range_finish<NW>(Q.R, (t0 + j) * Q.plane + row, status, nvalid_top, accw[j], accg[j], acct[j], red + j * NW * 6);
        }
    }
};

template <bool K8>
__global__ __launch_bounds__(FRISK_RANGE_NT) void panel_short_kernel(const PanelParams Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t tl[8];
    __shared__ double red[FRISK_PANEL_TILE * (FRISK_RANGE_NT / 64) * 6];
    ShortForm<K8> form(Q.R, lds, tl);
    uint16_t* mylist = reinterpret_cast<uint16_t*>(lds + panel_lds_list(form.kmin, form.kmax())) + (threadIdx.x >> 6) * FRISK_PANEL_LIST;
    range_row_loop(Q.R, form, PanelShortMode{Q, red, mylist});
}

__global__ __launch_bounds__(FRISK_RANGE_BIG_NT) void panel_long_kernel(const PanelParams Q, uint32_t* __restrict__ big, int64_t big_stride) {
    __shared__ uint32_t tl[8];
    __shared__ double red[FRISK_PANEL_TILE_LONG * (FRISK_RANGE_BIG_NT / 64) * 6];
    LongForm form(Q.R, big, big_stride, tl);
    range_row_loop(Q.R, form, PanelLongMode{Q, red});
}
