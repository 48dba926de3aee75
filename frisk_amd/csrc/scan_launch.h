// scan_launch.h - the scan kernels as frisk_abi.hip sees them: one plain function per kernel family, which takes the form that
// the schedule named (scan_forms.h), looks it up in the family's table and launches that instantiation; a form that is no row of
// the table is hipErrorInvalidValue, never a neighbouring kernel.  The kernels themselves are instantiated in scan_launch.hip
// (16-bit form, two-workgroup form, long-window form, the rows' scalar tail) and in scan8_launch.hip / scan8_launch4.hip /
// scan8_launch41.hip (narrow counters), so that the units compile side by side and an experiment on one kernel family rebuilds that
// family alone.  Every function enqueues on `st` and returns hipGetLastError() of its launch.
// Internal to the library: hidden, not part of the C ABI of include/frisk_hip.h.
#pragma once
#include "scan_forms.h"
#include "scan_params.h"

#define FRISK_INTERNAL __attribute__((visibility("hidden")))

// scan_launch.hip
// scan_kernel.h (16-bit counters, one or two workgroups per CU) over the candidates that P names
FRISK_INTERNAL hipError_t launch_scan16_form(const Scan16Form& form, const ScanParams& P, size_t lds, int grid, hipStream_t st);
// 32-bit tables of all orders in a global scratch slice per workgroup (scan_big_kernel.h)
FRISK_INTERNAL hipError_t launch_scan_big(const ScanParams& P, bool debug, int grid, uint32_t* big, int64_t stride, hipStream_t st);
// the rows' scalar tail behind the LDS kernels (finish_rows_kernel), 256 threads per block
FRISK_INTERNAL hipError_t launch_finish_rows(int grid, hipStream_t st, int64_t n, uint32_t* status, double* kld, double* gc,
                                             const double* sw, const double* sg);

// scan8_launch.hip
// one launch of scan8_kernel.h (narrow order-K counters): up to num_cu x the form's workgroups per CU, no more than work_items
FRISK_INTERNAL hipError_t launch_scan8_form(const Scan8Form& form, const ScanParams& P, int num_cu, int64_t work_items, hipStream_t st);
// the adaptive width's verdict (scan8_decide_kernel), one thread behind the sample
FRISK_INTERNAL hipError_t launch_scan8_decide(const unsigned int* counts, unsigned int n_sampled, int side_ok, unsigned int* verdict,
                                              hipStream_t st);
