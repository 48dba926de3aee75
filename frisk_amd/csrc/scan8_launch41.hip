// scan8_launch41.hip - the K = 8 bulk forms of scan8_kernel.h with 4-bit counters and the lowest order fixed at 1 (plain and side table,
// sliding or not): the other 4-bit rows of the form table (scan_forms.h) that launch_scan8_form (scan8_launch.hip) calls.  A unit of its own for build time alone:
// it compiles beside scan8_launch4.hip.  gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#include "scan8_launch.h"

FRISK_SCAN8_4BIT_KMIN1_FORMS(FRISK_SCAN8_INSTANTIATE)
