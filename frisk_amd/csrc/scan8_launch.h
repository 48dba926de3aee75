// scan8_launch.h - what the units of the narrow-counter kernels share: the launch of one scan8_kernel instantiation, and how a row of
// the form table (FRISK_SCAN8_FORMS, scan_forms.h) is instantiated.  scan8_launch4.hip and scan8_launch41.hip instantiate the two
// 4-bit sub-lists, scan8_launch.hip the 8-bit one; launch_scan8_form there calls them all.  The cut exists for build time alone: the
// units compile side by side.
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

// a row of the table as an instantiation of its launch: 256 threads, the logarithm table of 64 bins
#define FRISK_SCAN8_LAUNCH_OF(KMAX_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_) launch_scan8<KMAX_, 256, ITS_, BITS_, 64, WPS_, DBG_, ROLE_, SIDE_>
#define FRISK_SCAN8_INSTANTIATE(KMAX_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_) \
    template hipError_t FRISK_SCAN8_LAUNCH_OF(KMAX_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_)(const ScanParams&, int, int64_t, hipStream_t);
