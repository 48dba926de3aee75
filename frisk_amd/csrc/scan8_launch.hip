// scan8_launch.hip - the launches of scan8_kernel.h (narrow order-K counters, several workgroups per CU) and of the adaptive width's
// verdict: launch_narrow and launch_scan8_decide of scan_launch.h.  The 8-bit forms and K = 6, 7 are instantiated here, the 4-bit
// forms in scan8_launch4.hip and scan8_launch41.hip.  gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#include "scan8_launch.h"
#include "scan_schedule.h"          // FRISK_K7_WPS, FRISK_SIDE_SHARE

// (instantiated in scan8_launch4.hip and scan8_launch41.hip)
#define FRISK_SCAN8_4BIT_ELSEWHERE(ITS_, DBG_, ROLE_, SIDE_) extern FRISK_SCAN8_4BIT(ITS_, DBG_, ROLE_, SIDE_)
FRISK_SCAN8_4BIT_FORMS(FRISK_SCAN8_4BIT_ELSEWHERE)
#undef FRISK_SCAN8_4BIT_ELSEWHERE

// one launch of the narrow-counter K = 8 kernel: counter width, window class (<= 2048 / <= 5120 bases), debug dump
// (side: 4-bit counters with the side table for the period-4 max-mers)
hipError_t launch_narrow(int kmax, int bits, bool small_w, bool debug, const ScanParams& P, int num_cu, int64_t work_items, hipStream_t st,
                         bool sample, bool side, bool kmin1) {
    const bool slides = P.slide_pp > 0 && P.in_list == nullptr;        // (else: the instantiation without the ring, ROLE bit 1)
    // the 4-bit bulk forms with the lowest order compiled in (ROLE bit 2): the schedule asks for them, only a launch they exist for takes them
    if (kmin1 && !sample && bits == 4 && kmax == 8 && !debug && P.in_list == nullptr && P.kmin == 1) {
#define FRISK_L1(ITS_, SIDE_) return slides ? launch_scan8<8, 256, ITS_, 4, 64, 3, false, 4, SIDE_>(P, num_cu, work_items, st) \
                                            : launch_scan8<8, 256, ITS_, 4, 64, 3, false, 6, SIDE_>(P, num_cu, work_items, st)
        if (side) { if (small_w) FRISK_L1(8, true); FRISK_L1(20, true); }
        if (small_w) FRISK_L1(8, false);
        FRISK_L1(20, false);
#undef FRISK_L1
    }
    if (sample) {           // the sample of the adaptive width: 4-bit counters, its own name in kernel statistics; it runs the
                            // side-table form and counts what the plain form would have handed on as well
        if (small_w) return slides ? launch_scan8<8, 256, 8, 4, 64, 3, false, 1, true>(P, num_cu, work_items, st)
                                   : launch_scan8<8, 256, 8, 4, 64, 3, false, 3, true>(P, num_cu, work_items, st);
        return slides ? launch_scan8<8, 256, 20, 4, 64, 3, false, 1, true>(P, num_cu, work_items, st)
                      : launch_scan8<8, 256, 20, 4, 64, 3, false, 3, true>(P, num_cu, work_items, st);
    }
    if (side && P.in_list == nullptr && bits == 4 && kmax == 8 && !debug) {
        if (small_w) return slides ? launch_scan8<8, 256, 8, 4, 64, 3, false, 0, true>(P, num_cu, work_items, st)
                                   : launch_scan8<8, 256, 8, 4, 64, 3, false, 2, true>(P, num_cu, work_items, st);
        return slides ? launch_scan8<8, 256, 20, 4, 64, 3, false, 0, true>(P, num_cu, work_items, st)
                      : launch_scan8<8, 256, 20, 4, 64, 3, false, 2, true>(P, num_cu, work_items, st);
    }
#define FRISK_L7(K_, ITS_, DBG_) return launch_scan8<K_, 256, ITS_, 8, 64, FRISK_K7_WPS, DBG_>(P, num_cu, work_items, st)
    if (kmax == 7) {        // K = 6, 7: the 8-bit table is 16 / 4 KiB - registers, not LDS, bound the workgroups per CU
        if (debug) { if (small_w) FRISK_L7(7, 8, true); else FRISK_L7(7, 20, true); }
        if (small_w) FRISK_L7(7, 8, false);
        FRISK_L7(7, 20, false);
    }
    if (kmax == 6) {
        if (debug) { if (small_w) FRISK_L7(6, 8, true); else FRISK_L7(6, 20, true); }
        if (small_w) FRISK_L7(6, 8, false);
        FRISK_L7(6, 20, false);
    }
#undef FRISK_L7
#define FRISK_L8(ITS_, BITS_, WPS_, DBG_) return launch_scan8<8, 256, ITS_, BITS_, 64, WPS_, DBG_>(P, num_cu, work_items, st)
    if (bits == 4) {
        if (debug) { if (small_w) FRISK_L8(8, 4, 3, true); else FRISK_L8(20, 4, 3, true); }
        if (!slides) {
            if (small_w) return launch_scan8<8, 256, 8, 4, 64, 3, false, 2>(P, num_cu, work_items, st);
            return launch_scan8<8, 256, 20, 4, 64, 3, false, 2>(P, num_cu, work_items, st);
        }
        if (small_w) FRISK_L8(8, 4, 3, false);
        FRISK_L8(20, 4, 3, false);
    }
    if (debug) { if (small_w) FRISK_L8(8, 8, 2, true); else FRISK_L8(20, 8, 2, true); }
    if (small_w) FRISK_L8(8, 8, 2, false);
    FRISK_L8(20, 8, 2, false);
#undef FRISK_L8
}

// The adaptive width's verdict, on the device (one thread, behind the sample launch): which form scores the rest of the scan.
// counts[0] = sampled windows handed on anyway, [2] = scored, but a plain 4-bit counter would have wrapped, [3] = scored;
// n_sampled = windows in the sample.  The rule is frisk_abi.hip's (measured break-evens there): 8-bit bulk when more than three
// sampled windows in ten overflow 4 bits anyway; else the side table when the plain form would hand on more than side_share of
// the windows that are scored.  verdict[0] = 1 plain 4-bit, 2 4-bit + side table, 3 8-bit; verdict[1..3] = the three counts (for
// the host's statistics, read at the end of the scan).
__global__ void scan8_decide_kernel(const unsigned int* __restrict__ counts, unsigned int n_sampled, double side_share, int side_ok,
                                    unsigned int* __restrict__ verdict) {
    const unsigned int handed = counts[0], would = counts[2], scored = counts[3];
    unsigned int form = (double(handed) <= 0.3 * double(n_sampled)) ? 1u : 3u;
    if (form == 1u && side_ok && double(handed + would) > side_share * double(handed + scored)) form = 2u;
    verdict[0] = form; verdict[1] = handed; verdict[2] = would; verdict[3] = scored;
}

hipError_t launch_scan8_decide(const unsigned int* counts, unsigned int n_sampled, int side_ok, unsigned int* verdict, hipStream_t st) {
    scan8_decide_kernel<<<1, 1, 0, st>>>(counts, n_sampled, double(FRISK_SIDE_SHARE), side_ok, verdict);
    return hipGetLastError();
}
