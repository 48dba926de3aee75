// scan_launch.hip - the launches of scan_kernel.h (16-bit counters, one or two workgroups per CU: launch_scan16_form), of scan_big_kernel.h (long windows
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

// the row of FRISK_SCAN16_FORMS (scan_forms.h) that equals the form, and no other
hipError_t launch_scan16_form(const Scan16Form& form, const ScanParams& P, size_t lds, int grid, hipStream_t st) {
#define FRISK_SCAN16_ROW(NT_, K8_, ITS_, DBG_) \
    if (form == Scan16Form{NT_, K8_, ITS_, DBG_}) return launch_scan<NT_, K8_, ITS_, DBG_>(P, grid, lds, st);
    FRISK_SCAN16_FORMS(FRISK_SCAN16_ROW)
#undef FRISK_SCAN16_ROW
    return hipErrorInvalidValue;
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
