// ring_rows.h - where a position's genome-side value sits in a workgroup's slice of the ring (scan8_kernel.h, "THE GENOME-SIDE
// GATHER"): position p of the scaffold <-> row p % ITS, column p / ITS % FRISK8_RING_COLS, a double each, rows of FRISK8_RING_COLS
// doubles.  A window whose first base sits at row rb_r, column rb_q gives lane t its positions rb + t ITS + it, it < ITS: row
// rb_r + it, wrapped at ITS with a carry into the column.  Two forms of the same byte offset: the general one, and the one for
// windows that start on row 0 (rb_r = 0: no wrap, one column per lane).  No HIP here: the kernel includes this header, and
// tools/exp/ring_rows_host.cpp checks the two forms against each other on a CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FRISK_RING_FN __host__ __device__ inline
#else
#define FRISK_RING_FN inline
#endif

#define FRISK8_RING_COLS 256        // ring geometry: ITS rows x 256 columns of doubles per workgroup (position p <-> row p % ITS, column p / ITS % 256):
                                    // ITS x 256 = the most positions a window of this instantiation has - 40 KB per workgroup at 20 positions per lane
                                    // (round 3 had 512 columns, 80 KB: the same time, twice the footprint beside 4 MB of L2 per XCD)
#define FRISK8_RING_ROW_BYTES (FRISK8_RING_COLS * 8)

// the lane's column, in bytes, where the row index did not wrap (carry = 0) and where it did (carry = 1)
FRISK_RING_FN uint32_t ring_lane_col(uint32_t rb_q, uint32_t tid, uint32_t carry) {
    return ((rb_q + carry + tid) & (FRISK8_RING_COLS - 1u)) << 3;
}

// ---- the general form: any rb_r < ITS
// (uniform) slice + row of a lane's it-th position
template <int ITS>
FRISK_RING_FN uint32_t ring_uni_general(uint32_t slice_off, uint32_t rb_r, int it) {
    const uint32_t rr = rb_r + uint32_t(it);
    const uint32_t cy = rr >= uint32_t(ITS) ? 1u : 0u;
    return slice_off + (((rr - cy * uint32_t(ITS)) * FRISK8_RING_COLS) << 3);
}
// the lane's column: one of two values per window, by whether the row index wrapped
template <int ITS>
FRISK_RING_FN uint32_t ring_lane_general(uint32_t rb_r, int it, uint32_t lane_col0, uint32_t lane_col1) {
    return (rb_r + uint32_t(it) >= uint32_t(ITS)) ? lane_col1 : lane_col0;
}
template <int ITS>
FRISK_RING_FN uint32_t ring_off_general(uint32_t slice_off, uint32_t rb_r, uint32_t rb_q, uint32_t tid, int it) {
    return ring_uni_general<ITS>(slice_off, rb_r, it) +
           ring_lane_general<ITS>(rb_r, it, ring_lane_col(rb_q, tid, 0u), ring_lane_col(rb_q, tid, 1u));
}

// ---- the row-aligned form: rb_r = 0 (every window of a scan whose increment is a multiple of ITS): the row is `it`, the column
// never carries - a constant per position on top of one value per lane and window
FRISK_RING_FN uint32_t ring_uni_row0(uint32_t slice_off, int it) { return slice_off + uint32_t(it) * FRISK8_RING_ROW_BYTES; }
FRISK_RING_FN uint32_t ring_off_row0(uint32_t slice_off, uint32_t rb_q, uint32_t tid, int it) {
    return ring_uni_row0(slice_off, it) + ring_lane_col(rb_q, tid, 0u);
}

// ... as the scoring loop issues it (scan8_kernel.h, fetch()).  A wave whose lanes all read the ring: a scalar base at row
// ring_row0_base_row(it), which moves on before every fourth position (ring_row0_steps), the lane's column as the load's vector offset, and
// the rest of the row offset in the load's signed 13-bit immediate: -4096, -2048, 0, 2048.
#define FRISK8_RING_IMM_MIN (-4096)
#define FRISK8_RING_IMM_MAX 4095
FRISK_RING_FN constexpr int ring_row0_base_row(int it) { return (it & ~3) + 2; }
FRISK_RING_FN constexpr bool ring_row0_steps(int it) { return it > 0 && (it & 3) == 0; }
FRISK_RING_FN constexpr int ring_row0_imm(int it) { return (it - ring_row0_base_row(it)) * FRISK8_RING_ROW_BYTES; }
// A wave with lanes that gather: the lane's offset of row 0 - ring_off_row0(slice_off, rb_q, tid, 0), once per window - plus the row
FRISK_RING_FN uint32_t ring_row0_from_lane(uint32_t row0_lane, int it) { return row0_lane + uint32_t(it) * FRISK8_RING_ROW_BYTES; }
