// scan8_launch.h - what the two units of the narrow-counter kernels share: the launch of one scan8_kernel instantiation, and the list of
// the 4-bit forms, which scan8_launch4.hip and scan8_launch41.hip instantiate and scan8_launch.hip (launch_narrow, the 8-bit forms, K = 6 and 7) only calls.
// The cut is by counter width and exists for build time alone: the two halves compile side by side.
#pragma once
#include <algorithm>

#include "scan_launch.h"
#include "scan8_kernel.h"

template <int KMAX, int NT, int ITS, int BITS, int LOGN, int WPS, bool DEBUG, int ROLE = 0, bool SIDE = false>
FRISK_INTERNAL hipError_t launch_scan8(const ScanParams& P, int num_cu, int64_t work_items, hipStream_t st) {
    constexpr int wg_per_cu = WPS * 256 / NT;
    static_assert(Lds8<KMAX, BITS, LOGN, NT, SIDE>::granules * 1280 * wg_per_cu <= 160 * 1024, "the workgroups meant to share a CU must fit its LDS (allocated in pieces of 1280 bytes)");
    int grid = int(std::max<int64_t>(1, std::min<int64_t>(work_items, int64_t(num_cu) * wg_per_cu)));
    if (grid >= 8) grid &= ~7;
    scan8_kernel<KMAX, NT, ITS, BITS, LOGN, WPS, DEBUG, ROLE, SIDE><<<grid, NT, 0, st>>>(P);      // LDS is static (Lds8)
    return hipGetLastError();
}

// K = 8 with 4-bit counters, as X(ITS, DEBUG, ROLE, SIDE): the sample (ROLE bit 0) and the side-table form, each sliding or not (ROLE
// bit 1), then the plain form - debug, not sliding, sliding; FRISK_SCAN8_4BIT_KMIN1_FORMS: the bulk forms again with the lowest order
// fixed at 1 (ROLE bit 2; scan8_launch41.hip)
#define FRISK_SCAN8_4BIT_GENERIC_FORMS(X)                                                                                   \
    X(8, false, 1, true) X(8, false, 3, true) X(20, false, 1, true) X(20, false, 3, true)                                  \
    X(8, false, 0, true) X(8, false, 2, true) X(20, false, 0, true) X(20, false, 2, true)                                  \
    X(8, true, 0, false) X(20, true, 0, false) X(8, false, 2, false) X(20, false, 2, false) X(8, false, 0, false) X(20, false, 0, false)
#define FRISK_SCAN8_4BIT_KMIN1_FORMS(X)                                                                                     \
    X(8, false, 4, true) X(8, false, 6, true) X(20, false, 4, true) X(20, false, 6, true)                                  \
    X(8, false, 6, false) X(20, false, 6, false) X(8, false, 4, false) X(20, false, 4, false)
#define FRISK_SCAN8_4BIT_FORMS(X) FRISK_SCAN8_4BIT_GENERIC_FORMS(X) FRISK_SCAN8_4BIT_KMIN1_FORMS(X)
#define FRISK_SCAN8_4BIT(ITS_, DBG_, ROLE_, SIDE_) \
    template hipError_t launch_scan8<8, 256, ITS_, 4, 64, 3, DBG_, ROLE_, SIDE_>(const ScanParams&, int, int64_t, hipStream_t);
