// scan8_launch4.hip - the K = 8 forms of scan8_kernel.h with 4-bit counters and the lowest order as an argument (plain, side table, the
// adaptive width's sample): rows of the form table (scan_forms.h) that launch_scan8_form (scan8_launch.hip) calls.  gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#include "scan8_launch.h"

FRISK_SCAN8_4BIT_GENERIC_FORMS(FRISK_SCAN8_INSTANTIATE)
