// scan_launch.hip - the launches of scan_kernel.h (16-bit counters, one or two workgroups per CU), of scan_big_kernel.h (long windows
// and orders above 8) and of the rows' scalar tail: the functions of scan_launch.h that frisk_abi.hip calls.  gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#include "scan_launch.h"
#include "scan_kernel.h"
#include "scan_big_kernel.h"

// Per-row scalar tail of scan_kernel: KLD = sum Pw log2(Pw/Pg) = (T/Sw - ln Sw + ln Sg) / ln 2 (L453-454, L465-470), the GC
// fraction (L136) and the ZeroDivisionError flag of a max-mer without genome weight (L437).  Rows that were dropped by the
// N filter keep their NaNs.
__global__ __launch_bounds__(256) void finish_rows_kernel(int64_t n, uint32_t* __restrict__ status, double* __restrict__ kld,
                                                           double* __restrict__ gc, const double* __restrict__ sw,
                                                           const double* __restrict__ sg) {
    for (int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; row < n; row += int64_t(gridDim.x) * blockDim.x) {
        const uint32_t st = status[row];
        if (!(st & ROW_KEPT)) continue;
        const uint64_t packed = uint64_t(__double_as_longlong(gc[row]));
        gc[row] = double(uint32_t(packed)) / double(int64_t(packed >> 32));
        if (st & ROW_NO_MAXMER) { kld[row] = 0.0; continue; }
        const double Tt = kld[row], Sw = sw[row], Sg = sg[row];
        const double LN2 = 0.69314718055994530942;
        kld[row] = ((Tt / Sw - log(Sw)) + log(Sg)) / LN2;
        if (Sg != Sg) status[row] = st | ROW_ZERO_WEIGHT;
    }
}

namespace {

template <int NT, bool K8, int ITS, bool DEBUG>
hipError_t launch_scan(const ScanParams& P, int grid, size_t lds, hipStream_t st) {
    auto kern = scan_kernel<NT, K8, ITS, DEBUG>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       int(lds));
    if (e != hipSuccess) return e;
    kern<<<grid, NT, lds, st>>>(P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_scan16(const ScanParams& PP, int kmax, int its, bool debug, size_t lds, int g, hipStream_t st) {
    hipError_t le;
#define FRISK_LAUNCH16(NT_, K8_, ITS_, DBG_) le = launch_scan<NT_, K8_, ITS_, DBG_>(PP, g, lds, st)
    if (kmax == 8) {
        if (debug) { if (its) FRISK_LAUNCH16(512, true, 16, true); else FRISK_LAUNCH16(1024, true, 0, true); }
        else if (its == 4) FRISK_LAUNCH16(512, true, 4, false);
        else if (its == 10) FRISK_LAUNCH16(512, true, 10, false);
        else if (its == 16) FRISK_LAUNCH16(512, true, 16, false);
        else FRISK_LAUNCH16(1024, true, 0, false);
    } else {
        if (debug) { if (its) FRISK_LAUNCH16(512, false, 16, true); else FRISK_LAUNCH16(1024, false, 0, true); }
        else if (its == 4) FRISK_LAUNCH16(512, false, 4, false);
        else if (its == 10) FRISK_LAUNCH16(512, false, 10, false);
        else if (its == 16) FRISK_LAUNCH16(512, false, 16, false);
        else FRISK_LAUNCH16(1024, false, 0, false);
    }
#undef FRISK_LAUNCH16
    return le;
}

hipError_t launch_scan_two_wg(const ScanParams& P, int its, size_t lds, int grid, hipStream_t st) {
    if (its == 8) return launch_scan<256, false, 8, false>(P, grid, lds, st);
    return launch_scan<256, false, 20, false>(P, grid, lds, st);
}

hipError_t launch_scan_big(const ScanParams& P, bool debug, int grid, uint32_t* big, int64_t stride, hipStream_t st) {
    if (debug) scan_big_kernel<true><<<grid, FRISK_BIG_NT, 0, st>>>(P, big, stride);
    else scan_big_kernel<false><<<grid, FRISK_BIG_NT, 0, st>>>(P, big, stride);
    return hipGetLastError();
}

hipError_t launch_finish_rows(int grid, hipStream_t st, int64_t n, uint32_t* status, double* kld, double* gc, const double* sw,
                              const double* sg) {
    finish_rows_kernel<<<grid, 256, 0, st>>>(n, status, kld, gc, sw, sg);
    return hipGetLastError();
}
