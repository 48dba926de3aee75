// (CPU) the window geometry of scan8_kernel.h, checked on a CPU: frisk_amd/csrc/win_step.h holds a window's geometry computed from its
// candidate index (win_fresh) and advanced from its predecessor's by additions (win_next), and the 32-bit lane side of stage 1's
// sequence addressing.
//   * win_next == win_fresh, field by field, along 40 consecutive windows of a scaffold - every inc in 1..2600 (ITS = 8: below ITS x COLS,
//     win_next's precondition), every w in {600, 2000, 2048, 5000, 5120} that the instantiation holds, scaffolds placed so that the
//     resident position, the start inside the scaffold and the ring base straddle 2^32 and multiples of ITS x COLS;
//   * win_has_next is true exactly where the next candidate is a full window of the same scaffold that is no jump-back tail;
//   * the ring's place is the ring's definition: rb_q ITS + rb_r = st % (ITS COLS), rb_r < ITS;
//   * seq_base + seq_lane give the word indices and shift amounts of the 64-bit formulas, for every lane offset the kernel uses
//     (tid ITS, tid slide_pp) and every base offset 0..31, with bases on both sides of 2^32.
// Build: c++ -std=c++17 -O1 [-fsanitize=address,undefined] -Ifrisk_amd/csrc tools/exp/win_step_host.cpp -o win_step_host
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "ring_rows.h"
#include "win_step.h"

#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "win_step_host: %s failed: ", #cond);          \
            std::fprintf(stderr, __VA_ARGS__);                                  \
            std::fprintf(stderr, "\n");                                         \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static const int WS[] = {600, 2000, 2048, 5000, 5120};
constexpr int NWIN = 40;

template <int ITS>
static long check_walk(const WinScaf& d, int w, int inc) {
    constexpr int COLS = FRISK8_RING_COLS;
    const WinInc s = win_inc<ITS>(inc);
    CHECK(int64_t(s.q) * ITS + s.r == inc && s.r < uint32_t(ITS), "ITS %d inc %d: the increment's quotient and rest", ITS, inc);
    WinGeom g = win_fresh<ITS, COLS>(d, d.cand0, w, inc);
    long checked = 0;
    for (int i = 0; i < NWIN + 1; ++i) {
        const int64_t cand = d.cand0 + i;
        CHECK(uint64_t(g.rb_q) * ITS + g.rb_r == uint64_t(g.st) % uint64_t(ITS * COLS) && g.rb_r < uint32_t(ITS) && g.rb_q < uint32_t(COLS),
              "ITS %d w %d inc %d window %d: the ring's place (%u, %u) of st %lld", ITS, w, inc, i, g.rb_q, g.rb_r, (long long)g.st);
        CHECK(g.g0 == d.off + (g.st - d.base0), "ITS %d w %d inc %d window %d: resident position", ITS, w, inc, i);
        const bool more = win_has_next(d, g, cand, w, inc);
        if (i + 1 >= int(d.ncand)) { CHECK(!more, "ITS %d w %d inc %d: a successor behind the scaffold's last candidate", ITS, w, inc); break; }
        const WinGeom f = win_fresh<ITS, COLS>(d, cand + 1, w, inc);
        CHECK(more == (!g.jump && !f.jump && f.n == w), "ITS %d w %d inc %d window %d: win_has_next %d, the successor's jump %d n %d", ITS, w, inc, i,
              int(more), int(f.jump), f.n);
        if (more) {
            const WinGeom x = win_next<ITS, COLS>(g, s, w);
            CHECK(x.st == f.st, "ITS %d w %d inc %d window %d: st %lld, afresh %lld", ITS, w, inc, i + 1, (long long)x.st, (long long)f.st);
            CHECK(x.rep_start == f.rep_start && x.rep_stop == f.rep_stop, "ITS %d w %d inc %d window %d: reported %lld..%lld, afresh %lld..%lld", ITS, w, inc,
                  i + 1, (long long)x.rep_start, (long long)x.rep_stop, (long long)f.rep_start, (long long)f.rep_stop);
            CHECK(x.g0 == f.g0, "ITS %d w %d inc %d window %d: g0 %lld, afresh %lld", ITS, w, inc, i + 1, (long long)x.g0, (long long)f.g0);
            CHECK(x.n == f.n && x.jump == f.jump, "ITS %d w %d inc %d window %d: n %d jump %d, afresh %d %d", ITS, w, inc, i + 1, x.n, int(x.jump), f.n, int(f.jump));
            CHECK(x.rb_q == f.rb_q && x.rb_r == f.rb_r, "ITS %d w %d inc %d window %d: ring (%u, %u), afresh (%u, %u)", ITS, w, inc, i + 1, x.rb_q, x.rb_r,
                  f.rb_q, f.rb_r);
            g = x;              // (the kernel's chain: every window of the walk from its predecessor)
            ++checked;
        } else {
            g = f;
        }
    }
    return checked;
}

template <int ITS>
static long check_geometry() {
    constexpr int64_t RING = int64_t(ITS) * FRISK8_RING_COLS;
    constexpr int64_t TWO32 = int64_t(1) << 32;
    long checked = 0;
    for (int w : WS) {
        if (w > RING) continue;                 // (longer windows than this instantiation's lanes cover)
        for (int inc = 1; inc <= 2600 && inc < RING; ++inc) {
            // window index of the scaffold's first candidate: 0; the walk's start inside the scaffold straddles 2^32; ... a multiple of
            // ITS x COLS far from 0; (streamed pieces: base0 > 0, the first candidates' bases already gone)
            const int64_t j0s[4] = {0, TWO32 / inc - NWIN / 2, (7 * RING * 1000003) / inc - NWIN / 2, 3};
            const int64_t offs[4] = {TWO32 - int64_t(NWIN / 2) * inc - 5, 12345, 0, TWO32 * 2 + 77};
            for (int k = 0; k < 4; ++k) {
                WinScaf d;
                d.kind = 0;
                d.j0 = j0s[k] < 0 ? 0 : j0s[k];
                d.cand0 = 1000 * k + 3;
                d.ncand = NWIN + 1;
                // windows 0 .. NWIN - 1 are full, the last candidate is a jump-back tail
                d.size = (d.j0 + NWIN - 1) * inc + w + inc / 2;
                d.base0 = k == 3 ? 3 * int64_t(inc) - 1 : (d.j0 * inc > 11 ? d.j0 * inc - 11 : 0);
                d.off = offs[k];
                const long got = check_walk<ITS>(d, w, inc);
                CHECK(got == NWIN - 1, "ITS %d w %d inc %d placement %d: %ld successors checked", ITS, w, inc, k, got);
                checked += got;
            }
            // a whole-scaffold window (kind 1) and a scaffold shorter than a window have no successor
            WinScaf d1;
            d1.kind = 1; d1.j0 = 0; d1.cand0 = 5; d1.ncand = 1; d1.size = w + w / 2; d1.base0 = 0; d1.off = TWO32 - 9;
            const WinGeom g1 = win_fresh<ITS, FRISK8_RING_COLS>(d1, 5, w, inc);
            CHECK(g1.st == 0 && g1.n == w + w / 2 && g1.rep_start == 1 && g1.rep_stop == d1.size && !win_has_next(d1, g1, 5, w, inc), "kind 1");
            d1.kind = 0; d1.size = w - 1;
            const WinGeom g2 = win_fresh<ITS, FRISK8_RING_COLS>(d1, 5, w, inc);
            CHECK(g2.jump && g2.st >= 0 && g2.n <= w && !win_has_next(d1, g2, 5, w, inc), "a scaffold shorter than a window");
        }
    }
    return checked;
}

// the lane's word indices and shifts: 32-bit arithmetic on (g & 31) + off against the 64-bit formulas
static long check_lanes() {
    const uint64_t words[] = {0, 5, (uint64_t(1) << 27) - 1, uint64_t(1) << 27, (uint64_t(1) << 27) + 1, uint64_t(1) << 40};
    long checked = 0;
    for (uint64_t wd : words)
        for (uint32_t bit = 0; bit < 32; ++bit) {
            const int64_t g = int64_t(wd * 32 + bit);
            const SeqBase b = seq_base(g);
            CHECK(b.word == wd && b.bit == bit, "base %lld: word %llu bit %u", (long long)g, (unsigned long long)b.word, b.bit);
            for (uint32_t tid = 0; tid < 256; ++tid)
                for (uint32_t per = 0; per <= 20; ++per) {       // tid ITS (8, 20) and tid slide_pp (1 .. 11 at inc <= 2600); 0: a clamped lane
                    const uint32_t off = tid * per;
                    const SeqLane l = seq_lane(b, off);
                    const int64_t gl = g + int64_t(off);
                    CHECK(int64_t(2 * b.word + l.cw) == (gl >> 4) && int64_t(b.word + l.mw) == (gl >> 5), "base %lld offset %u: words", (long long)g, off);
                    CHECK(l.shc == 32 - int(gl & 15) * 2 && l.shm == 32 - int(gl & 31), "base %lld offset %u: shifts %d %d", (long long)g, off, l.shc, l.shm);
                    CHECK(l.shc >= 2 && l.shc <= 32 && l.shm >= 1 && l.shm <= 32, "base %lld offset %u: shift amounts in range", (long long)g, off);
                    ++checked;
                }
        }
    return checked;
}

int main() {
    const long a = check_geometry<20>();
    const long b = check_geometry<8>();
    const long c = check_lanes();
    std::printf("win_step_host ok: %ld + %ld successors, %ld lane offsets checked\n", a, b, c);
    return 0;
}
