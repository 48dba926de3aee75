// (CPU) which scans take the K = 8 4-bit bulk kernels compiled for the lowest order 1 (scan8_kernel.h, SCAN8_ROLE_KMIN1): plan_scan_schedule's
// statement ScanSchedule::kmin1_form over a sweep of shapes - lowest order 1..5, highest order 6..8, both counter widths and the
// adaptive choice (flags, the batch's hint, a scan long enough to sample), FRISK_SCAN_GENERIC on and off, the debug dump on and off,
// windows of both classes and one beyond the narrow-counter kernels, sliding and not.  The form is named exactly where K = 8, kmin = 1,
// no debug dump and no FRISK_SCAN_GENERIC meet on the narrow-counter path, and nowhere else; nothing else of a schedule depends on the flag.
// Build: c++ -std=c++17 -O1 [-fsanitize=address,undefined] -Ifrisk_amd/csrc tools/exp/scan_dispatch_host.cpp -o scan_dispatch_host
#include <cstdio>
#include <cstring>

#include "scan_schedule.h"

static long fails = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++fails <= 20) {                                                \
                std::fprintf(stderr, "scan_dispatch_host: %s failed: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);                              \
                std::fprintf(stderr, "\n");                                     \
            }                                                                   \
        }                                                                       \
    } while (0)

// an upper bound of scan_kernel.h's LDS (make_layout at kmin = 1): the decisions under test do not read it below 160 KB
static uint32_t lds_of(int K, int64_t maxwin, int lv) {
    int64_t bins = 0;
    for (int k = 1; k <= (K == 8 ? 6 : K); ++k) bins += int64_t(1) << (2 * k);
    int64_t o = (K == 8 ? 131072 : 0) + (bins * 2 + 15) / 16 * 16;
    if (K == 8) o += (scan_orphan_cap(maxwin) * 2 + 15) / 16 * 16;
    if (lv) o += 1024 * 8 + 1024 * 4;
    return uint32_t(o + 16 * 8 + 128 * 16 + (2 * 16 * 4 + 16 * 6 * 8));
}

int main() {
    long plans = 0, named = 0, named_with_4bit_bulk = 0;
    const uint32_t widths[] = {0u, FRISK_SCAN_BITS4, FRISK_SCAN_SIDE4};
    const int hints[][2] = {{0, 0}, {4, 0}, {4, 1}, {8, 0}};
    const int64_t ns[] = {1, 43, 12063, 410000, 3058000};
    for (int kmin = 1; kmin <= 5; ++kmin) for (int K = 6; K <= 8; ++K) for (int64_t n : ns) for (int w : {2048, 5000, 5121})
    for (int inc : {w / 5, w / 2 + 1}) for (uint32_t width : widths) for (const auto& h : hints)
    for (uint32_t chunks : {0u, uint32_t(FRISK_SCAN_CHUNKS)}) for (int debug = 0; debug < 2; ++debug) for (int generic = 0; generic < 2; ++generic) {
        ScanShape s = ScanShape();
        s.kmin = kmin; s.kmax = K; s.num_cu = 256; s.n = n; s.w = w; s.inc = inc; s.plan_maxwin = w; s.debug = debug != 0;
        s.flags = width | chunks | (generic ? FRISK_SCAN_GENERIC : 0u);
        s.width_hint = h[0]; s.hint_side = h[1]; s.hint_matches = true;
        s.lv_shared = kmin <= 5 ? 5 : 0;
        s.lds_shared = lds_of(K, w, s.lv_shared); s.lds_level0 = lds_of(K, w, 0);
        const ScanSchedule S = plan_scan_schedule(s);
        ++plans;
        CHECK(S.error == nullptr, "kmin %d K %d n %ld w %d inc %d flags %u", kmin, K, long(n), w, inc, s.flags);
        // the narrow-counter kernels take windows up to 5120 bases; kmin <= K - 3 (the shared prefix level)
        const bool narrow_path = S.path == SCAN_PATH_NARROW;
        CHECK(narrow_path == (w <= 5120 && kmin <= K - 3), "kmin %d K %d w %d", kmin, K, w);
        const bool want = narrow_path && K == 8 && kmin == 1 && !debug && !generic;
        CHECK(S.kmin1_form == want, "kmin %d K %d n %ld w %d inc %d flags %u debug %d hint %d: kmin1_form %d", kmin, K, long(n), w, inc,
              s.flags, debug, h[0], int(S.kmin1_form));
        if (S.kmin1_form) {
            ++named;
            CHECK(S.narrow8 && !s.debug, "the form exists at K = 8 without the debug dump");
            if (S.bulk == 4) ++named_with_4bit_bulk;
        }
        // the flag asks for another instantiation of the same kernel and for nothing else
        if (generic) {
            ScanShape t = s;
            t.flags &= ~uint32_t(FRISK_SCAN_GENERIC);
            ScanSchedule T = plan_scan_schedule(t);
            T.kmin1_form = S.kmin1_form;
            CHECK(T.path == S.path && T.bulk == S.bulk && T.side == S.side && T.sample == S.sample && T.chunk8 == S.chunk8 &&
                  T.slide_pp == S.slide_pp && T.ring_slices == S.ring_slices && T.dealt == S.dealt && T.cut == S.cut &&
                  T.sel_mod == S.sel_mod && T.sel_mode == S.sel_mode && T.nsample == S.nsample && T.segments == S.segments &&
                  T.short_scan == S.short_scan && T.small_w == S.small_w && T.grid == S.grid && T.chunk == S.chunk,
                  "FRISK_SCAN_GENERIC moved the schedule: kmin %d K %d n %ld w %d inc %d flags %u", kmin, K, long(n), w, inc, s.flags);
        }
    }
    // the flagship: one rank's C5 scan (k = 1..8, w = 5000, inc = 1000) samples, then runs the 4-bit bulk compiled for kmin = 1
    {
        ScanShape s = ScanShape();
        s.kmin = 1; s.kmax = 8; s.num_cu = 256; s.n = 3058000; s.w = 5000; s.inc = 1000; s.plan_maxwin = 5000;
        s.lv_shared = 5; s.lds_shared = lds_of(8, 5000, 5); s.lds_level0 = lds_of(8, 5000, 0);
        const ScanSchedule S = plan_scan_schedule(s);
        CHECK(S.error == nullptr && S.path == SCAN_PATH_NARROW && S.sample && S.bulk == 4 && S.kmin1_form && S.slide_pp == 4, "flagship");
        s.width_hint = 4; s.hint_matches = true;
        const ScanSchedule H = plan_scan_schedule(s);
        CHECK(H.error == nullptr && !H.sample && H.bulk == 4 && !H.side && H.kmin1_form, "flagship, hinted");
    }
    CHECK(named > 0 && named_with_4bit_bulk > 0 && named < plans, "the sweep reaches both answers");
    if (fails) { std::fprintf(stderr, "scan_dispatch_host: %ld checks failed\n", fails); return 1; }
    std::printf("scan_dispatch_host ok: %ld schedules, %ld name the kmin = 1 form (%ld of them with a 4-bit bulk)\n", plans, named, named_with_4bit_bulk);
    return 0;
}
