// (CPU) the ring's address arithmetic of scan8_kernel.h, checked exhaustively: frisk_amd/csrc/ring_rows.h holds the general form of a
// position's byte offset in a workgroup's slice and the row-aligned form that windows with rb_r = 0 take.
//   * rb_r = 0: both forms give the same offset for every it < ITS, tid < 256, rb_q < FRISK8_RING_COLS - and so do the two shapes in which
//     the scoring loop issues the row-aligned form: a scalar base that moves along + the lane's column + an immediate that fits the load's
//     signed 13 bits, and the lane's offset of row 0 + the row;
//   * every rb_r: the general form is the ring's definition - position p = rb + tid ITS + it <-> row p % ITS, column p / ITS % COLS;
//   * rb_r = 1..ITS-1: no two positions of a window share a slot, and every slot lies inside the slice.
// Build: c++ -std=c++17 -O1 [-fsanitize=address,undefined] -Ifrisk_amd/csrc tools/exp/ring_rows_host.cpp -o ring_rows_host
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ring_rows.h"

#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "ring_rows_host: %s failed: ", #cond);         \
            std::fprintf(stderr, __VA_ARGS__);                                  \
            std::fprintf(stderr, "\n");                                         \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

template <int ITS>
static long check_its() {
    constexpr uint32_t NT = 256, COLS = FRISK8_RING_COLS;
    constexpr uint32_t slice_bytes = uint32_t(ITS) * COLS * 8u;
    // (a slice offset like the kernel's: the genome table of 4^8 doubles, then whole slices with their padding)
    const uint32_t slice_off = (65536u + 7u * (uint32_t(ITS) * COLS + 16u)) * 8u;
    long checked = 0;
    // rb_r = 0: the row-aligned form is the general form
    for (uint32_t rb_q = 0; rb_q < COLS; ++rb_q)
        for (uint32_t tid = 0; tid < NT; ++tid) {
            // (the kernel's scalar base: set up once per window, moved on where ring_row0_steps says so)
            int64_t base = int64_t(slice_off) + ring_row0_base_row(0) * FRISK8_RING_ROW_BYTES;
            const uint32_t row0_lane = ring_off_row0(slice_off, rb_q, tid, 0);
            for (int it = 0; it < ITS; ++it) {
                const uint32_t g = ring_off_general<ITS>(slice_off, 0u, rb_q, tid, it);
                if (ring_row0_steps(it)) base += (ring_row0_base_row(it) - ring_row0_base_row(it - 1)) * FRISK8_RING_ROW_BYTES;
                const int imm = ring_row0_imm(it);
                CHECK(imm >= FRISK8_RING_IMM_MIN && imm <= FRISK8_RING_IMM_MAX, "ITS %d it %d: immediate %d outside 13 signed bits", ITS, it, imm);
                CHECK(base == int64_t(slice_off) + int64_t(ring_row0_base_row(it)) * FRISK8_RING_ROW_BYTES, "ITS %d it %d: the moving base", ITS, it);
                CHECK(base + int64_t(ring_lane_col(rb_q, tid, 0u)) + imm == int64_t(g), "ITS %d rb_q %u tid %u it %d: base + column + immediate %lld, general %u",
                      ITS, rb_q, tid, it, (long long)(base + int64_t(ring_lane_col(rb_q, tid, 0u)) + imm), g);
                CHECK(ring_row0_from_lane(row0_lane, it) == g, "ITS %d rb_q %u tid %u it %d: lane offset + row %u, general %u", ITS, rb_q, tid, it,
                      ring_row0_from_lane(row0_lane, it), g);
                const uint32_t r = ring_off_row0(slice_off, rb_q, tid, it);
                CHECK(g == r, "ITS %d rb_q %u tid %u it %d: general %u, row-aligned %u", ITS, rb_q, tid, it, g, r);
                CHECK(ring_uni_general<ITS>(slice_off, 0u, it) == ring_uni_row0(slice_off, it), "ITS %d it %d: uniform part", ITS, it);
                CHECK(ring_lane_general<ITS>(0u, it, 1u, 2u) == 1u, "ITS %d it %d: the column carried at rb_r = 0", ITS, it);
                ++checked;
            }
        }
    // every rb_r: the general form against the ring's definition; no slot twice in a window; every slot inside the slice
    std::vector<uint32_t> owner(static_cast<size_t>(ITS) * COLS);
    for (uint32_t rb_r = 0; rb_r < uint32_t(ITS); ++rb_r)
        for (uint32_t rb_q = 0; rb_q < COLS; ++rb_q) {
            owner.assign(owner.size(), 0u);
            const uint32_t rb = rb_q * uint32_t(ITS) + rb_r;
            for (uint32_t tid = 0; tid < NT; ++tid)
                for (int it = 0; it < ITS; ++it) {
                    const uint32_t p = rb + tid * uint32_t(ITS) + uint32_t(it);
                    const uint32_t want = slice_off + ((p % uint32_t(ITS)) * COLS + (p / uint32_t(ITS)) % COLS) * 8u;
                    const uint32_t g = ring_off_general<ITS>(slice_off, rb_r, rb_q, tid, it);
                    CHECK(g == want, "ITS %d rb_r %u rb_q %u tid %u it %d: general %u, definition %u", ITS, rb_r, rb_q, tid, it, g, want);
                    CHECK(g >= slice_off && g - slice_off < slice_bytes && (g & 7u) == 0u, "ITS %d rb_r %u rb_q %u tid %u it %d: offset %u outside the slice",
                          ITS, rb_r, rb_q, tid, it, g);
                    uint32_t& o = owner[(g - slice_off) >> 3];
                    CHECK(o == 0u, "ITS %d rb_r %u rb_q %u: positions %u and %u share a slot", ITS, rb_r, rb_q, o - 1u, tid * uint32_t(ITS) + uint32_t(it));
                    o = tid * uint32_t(ITS) + uint32_t(it) + 1u;
                    ++checked;
                }
        }
    return checked;
}

int main() {
    const long a = check_its<20>();
    const long b = check_its<8>();
    std::printf("ring_rows_host ok: %ld + %ld offsets checked\n", a, b);
    return 0;
}
