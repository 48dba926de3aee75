// scan_launch.h - the scan kernels as frisk_abi.hip sees them: one plain function per launch.  The kernels themselves are
// instantiated in scan_launch.hip (16-bit form, two-workgroup form, long-window form, the rows' scalar tail) and in
// scan8_launch.hip / scan8_launch4.hip / scan8_launch41.hip (narrow counters), so that the units compile side by side and an experiment on one
// kernel family rebuilds that family alone.  Every function enqueues on `st` and returns hipGetLastError() of its launch.
// Internal to the library: hidden, not part of the C ABI of include/frisk_hip.h.
#pragma once
#include "scan_params.h"

#define FRISK_INTERNAL __attribute__((visibility("hidden")))

// scan_launch.hip
// the 16-bit form (scan_kernel.h) over the candidates that P names, by highest order, window class (its) and debug dump
FRISK_INTERNAL hipError_t launch_scan16(const ScanParams& P, int kmax, int its, bool debug, size_t lds, int grid, hipStream_t st);
// the same with two 256-thread workgroups per CU (kmax <= 7; its = 8 or 20)
FRISK_INTERNAL hipError_t launch_scan_two_wg(const ScanParams& P, int its, size_t lds, int grid, hipStream_t st);
// 32-bit tables of all orders in a global scratch slice per workgroup (scan_big_kernel.h)
FRISK_INTERNAL hipError_t launch_scan_big(const ScanParams& P, bool debug, int grid, uint32_t* big, int64_t stride, hipStream_t st);
// the rows' scalar tail behind the LDS kernels (finish_rows_kernel), 256 threads per block
FRISK_INTERNAL hipError_t launch_finish_rows(int grid, hipStream_t st, int64_t n, uint32_t* status, double* kld, double* gc,
                                             const double* sw, const double* sg);

// scan8_launch.hip
// one launch of the narrow-counter K = 8 kernel: counter width, window class (<= 2048 / <= 5120 bases), debug dump
// (side: 4-bit counters with the side table for the period-4 max-mers; kmin1: the 4-bit bulk form compiled for the lowest order 1 -
//  ScanSchedule::kmin1_form says when)
FRISK_INTERNAL hipError_t launch_narrow(int kmax, int bits, bool small_w, bool debug, const ScanParams& P, int num_cu, int64_t work_items,
                                        hipStream_t st, bool sample = false, bool side = false, bool kmin1 = false);
// the adaptive width's verdict (scan8_decide_kernel), one thread behind the sample
FRISK_INTERNAL hipError_t launch_scan8_decide(const unsigned int* counts, unsigned int n_sampled, int side_ok, unsigned int* verdict,
                                              hipStream_t st);
