// win_step.h - the geometry of a scan window (scan8_kernel.h): where candidate `cand` of a scaffold starts, what it reports, where it
// sits in the resident batch and in the workgroup's ring - computed from the candidate index (win_fresh, crawlGenome L211-245) or, for
// the successor of a window inside a chunk, from its predecessor by additions (win_next).  Fifteen of sixteen windows of a chunk are
// such successors: the multiplies, the 64-bit modulo and the divisions of win_fresh then run once per chunk instead of once per window.
// And the lane side of stage 1's sequence addressing: a uniform 64-bit word index plus 32-bit arithmetic on (g & 31) + the lane's offset.
// No HIP here: the kernel includes this header, and tools/exp/win_step_host.cpp checks win_next against win_fresh and the 32-bit lane
// arithmetic against the 64-bit formulas on a CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FRISK_WIN_FN __host__ __device__ inline
#else
#define FRISK_WIN_FN inline
#endif

// what the geometry reads of a scaffold's descriptor (ScafDesc)
struct WinScaf {
    int64_t off, size, base0;       // resident position of the scaffold's base `base0`; its length in bases
    int64_t cand0, ncand, j0;       // its candidates [cand0, cand0 + ncand); the window index of the first of them
    int32_t kind;                   // 1: the whole scaffold is one window (a rescued small scaffold, L219)
};

struct WinGeom {
    int64_t st;                     // first base of the window in its scaffold
    int64_t rep_start, rep_stop;    // reported coordinates
    int64_t g0;                     // resident position of the first base
    int32_t n;                      // bases
    bool jump;                      // a jump-back tail (L230-232)
    uint32_t rb_q, rb_r;            // the first base's place in the ring: st % (ITS COLS) = rb_q ITS + rb_r, rb_r < ITS (ring_rows.h)
};

// the increment as win_next adds it: per-launch constants
struct WinInc {
    int32_t inc;
    uint32_t q, r;                  // inc / ITS, inc % ITS
};
template <int ITS>
FRISK_WIN_FN WinInc win_inc(int32_t inc) {
    WinInc s;
    s.inc = inc; s.q = uint32_t(inc) / uint32_t(ITS); s.r = uint32_t(inc) - s.q * uint32_t(ITS);
    return s;
}

// candidate `cand` of scaffold `d`, from scratch
template <int ITS, int COLS>
FRISK_WIN_FN WinGeom win_fresh(const WinScaf& d, int64_t cand, int32_t w, int32_t inc) {
    WinGeom g;
    const int64_t j = cand - d.cand0 + d.j0;               // window index inside the scaffold
    g.jump = false;
    if (d.kind == 1) { g.st = 0; g.n = int32_t(d.size); g.rep_start = 1; g.rep_stop = d.size; }      // L219
    else {
        g.st = j * inc;
        g.n = w;
        g.rep_start = g.st + 1; g.rep_stop = g.st + w;                                      // L245
        if (g.st + w > d.size) {                                                            // L230-232
            g.jump = true;
            g.st = d.size - w;
            g.rep_start = g.st; g.rep_stop = d.size;                                        // L243: 0-based start
            if (g.st < 0) { g.st += d.size; if (g.st < 0) g.st = 0; }                       // negative slice start
            g.n = int32_t(d.size - g.st);
        }
    }
    g.g0 = d.off + (g.st - d.base0);
    const uint32_t ring_base = uint32_t(uint64_t(g.st) % uint64_t(ITS * COLS));
    g.rb_q = ring_base / uint32_t(ITS);
    g.rb_r = ring_base - g.rb_q * uint32_t(ITS);
    return g;
}

// whether the successor of `g` - candidate cand + 1 - is win_next's: in the same scaffold, a full window like this one, no jump-back
FRISK_WIN_FN bool win_has_next(const WinScaf& d, const WinGeom& g, int64_t cand, int32_t w, int32_t inc) {
    return d.kind == 0 && !g.jump && cand + 1 < d.cand0 + d.ncand && g.st + int64_t(inc) + w <= d.size;
}

// the successor of a window with win_has_next: additions only.  The ring's row moves on by inc % ITS with a carry into the column, the
// column by inc / ITS, wrapped at COLS (inc < w <= ITS COLS, so one subtraction each)
// (a full window that is no jump-back tail reports st + 1 .. st + w, and so does its successor: nothing of that is carried)
template <int ITS, int COLS>
FRISK_WIN_FN WinGeom win_next(const WinGeom& p, const WinInc& s, int32_t w) {
    WinGeom g;
    g.st = p.st + s.inc;
    g.rep_start = g.st + 1; g.rep_stop = g.st + w;
    g.g0 = p.g0 + s.inc;
    g.n = w;
    g.jump = false;
    uint32_t r = p.rb_r + s.r, q = p.rb_q + s.q;
    if (r >= uint32_t(ITS)) { r -= uint32_t(ITS); ++q; }
    if (q >= uint32_t(COLS)) q -= uint32_t(COLS);
    g.rb_q = q; g.rb_r = r;
    return g;
}

// ---- stage 1's sequence addressing.  A lane reads 32 bases from resident position g + off, off its own 32-bit offset: three 16-base
// code words from word (g + off) >> 4, funnel-shifted by 32 - 2 ((g + off) & 15), and two 32-base mask words from word (g + off) >> 5,
// shifted by 32 - ((g + off) & 31).  With g = 32 (g >> 5) + (g & 31) the 64-bit part - g >> 5 - is uniform, and the lane's word
// indices and shift amounts follow from x = (g & 31) + off in 32 bits.
struct SeqBase {
    uint64_t word;                  // (uniform) g >> 5: index of the 32-base mask word; twice that: of the 16-base code word
    uint32_t bit;                   // (uniform) g & 31
};
FRISK_WIN_FN SeqBase seq_base(int64_t g) {
    SeqBase b;
    b.word = uint64_t(g) >> 5; b.bit = uint32_t(uint64_t(g)) & 31u;
    return b;
}
struct SeqLane {
    uint32_t cw, mw;                // code / mask word index, on top of 2 word / word
    int shc, shm;                   // the two shift amounts
};
FRISK_WIN_FN SeqLane seq_lane(const SeqBase& b, uint32_t off) {
    const uint32_t x = b.bit + off;
    SeqLane l;
    l.cw = x >> 4; l.mw = x >> 5;
    l.shc = 32 - int(x & 15u) * 2; l.shm = 32 - int(x & 31u);
    return l;
}
