// scan8_launch.hip - the launches of scan8_kernel.h (narrow order-K counters, several workgroups per CU) and of the adaptive width's
// verdict: launch_scan8_form and launch_scan8_decide of scan_launch.h.  The 8-bit forms (K = 8, 7 and 6) are instantiated here, the
// 4-bit forms in scan8_launch4.hip and scan8_launch41.hip.  gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#include "scan8_launch.h"
#include "scan_schedule.h"          // FRISK_SIDE_SHARE

FRISK_SCAN8_8BIT_FORMS(FRISK_SCAN8_INSTANTIATE)
// (instantiated in scan8_launch4.hip and scan8_launch41.hip)
#define FRISK_SCAN8_ELSEWHERE(...) extern FRISK_SCAN8_INSTANTIATE(__VA_ARGS__)
FRISK_SCAN8_4BIT_GENERIC_FORMS(FRISK_SCAN8_ELSEWHERE)
FRISK_SCAN8_4BIT_KMIN1_FORMS(FRISK_SCAN8_ELSEWHERE)
#undef FRISK_SCAN8_ELSEWHERE

// one launch of the narrow-counter kernel: the table's row that equals the form, and no other
hipError_t launch_scan8_form(const Scan8Form& form, const ScanParams& P, int num_cu, int64_t work_items, hipStream_t st) {
#define FRISK_SCAN8_ROW(KMAX_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_)          \
    if (form == Scan8Form{KMAX_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_})       \
        return FRISK_SCAN8_LAUNCH_OF(KMAX_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_)(P, num_cu, work_items, st);
    FRISK_SCAN8_FORMS(FRISK_SCAN8_ROW)
#undef FRISK_SCAN8_ROW
    return hipErrorInvalidValue;
}

// The adaptive width's verdict, on the device (one thread, behind the sample launch): which form scores the rest of the scan.
// counts: the counter block of the sample's segment (scan_params.h) - SCAN_CNT_LIST1 = sampled windows handed on anyway,
// SCAN_CNT_SAMPLE_WOULD = scored, but a plain 4-bit counter would have wrapped, SCAN_CNT_SAMPLE_SCORED = scored; n_sampled = windows in the sample.  The rule is frisk_abi.hip's (measured break-evens there): 8-bit bulk when more than three
// sampled windows in ten overflow 4 bits anyway; else the side table when the plain form would hand on more than side_share of
// the windows that are scored.  verdict[0] = 1 plain 4-bit, 2 4-bit + side table, 3 8-bit; verdict[1..3] = the three counts (for
// the host's statistics, read at the end of the scan).
__global__ void scan8_decide_kernel(const unsigned int* __restrict__ counts, unsigned int n_sampled, double side_share, int side_ok,
                                    unsigned int* __restrict__ verdict) {
    const unsigned int handed = counts[SCAN_CNT_LIST1], would = counts[SCAN_CNT_SAMPLE_WOULD], scored = counts[SCAN_CNT_SAMPLE_SCORED];
    unsigned int form = (double(handed) <= 0.3 * double(n_sampled)) ? 1u : 3u;
    if (form == 1u && side_ok && double(handed + would) > side_share * double(handed + scored)) form = 2u;
    verdict[0] = form; verdict[1] = handed; verdict[2] = would; verdict[3] = scored;
}

hipError_t launch_scan8_decide(const unsigned int* counts, unsigned int n_sampled, int side_ok, unsigned int* verdict, hipStream_t st) {
    scan8_decide_kernel<<<1, 1, 0, st>>>(counts, n_sampled, double(FRISK_SIDE_SHARE), side_ok, verdict);
    return hipGetLastError();
}
