// scan_forms.h - which instantiation of a scan kernel a launch runs, as a plain value: the template arguments of scan8_kernel
// (Scan8Form) and of scan_kernel (Scan16Form) that vary, the rule that names the form of one launch, and one table per kernel family
// of the instantiations that exist.  plan_scan_schedule (scan_schedule.h) names the form of every launch of a scan by the rule; the
// launchers (scan8_launch.hip, scan_launch.hip) look a form up in the table and refuse one that is no row of it.  No HIP here: the
// kernels read the role names, tools/exp/scan_forms_host.cpp checks rule and tables on a CPU.
#pragma once

#define FRISK_K7_WPS 4              // waves per SIMD (= 256-thread workgroups per CU) of the K = 6, 7 narrow-counter kernels

// scan8_kernel's ROLE, a set of bits
enum {
    SCAN8_ROLE_SAMPLE = 1,          // the sample of the adaptive width (a name of its own in kernel statistics; with SIDE it counts what the plain form would have handed on)
    SCAN8_ROLE_NO_SLIDE = 2,        // no window of the launch slides, hence no ring
    SCAN8_ROLE_KMIN1 = 4            // the lowest order is the constant 1, not the argument (the K = 8 4-bit bulk forms)
};

// scan8_kernel<kmax, 256, its, bits, 64, wps, debug, role, side>; kmax == 0: no form
struct Scan8Form {
    int kmax, its, bits, wps;
    bool debug;
    int role;
    bool side;
};
inline bool operator==(const Scan8Form& a, const Scan8Form& b) {
    return a.kmax == b.kmax && a.its == b.its && a.bits == b.bits && a.wps == b.wps && a.debug == b.debug && a.role == b.role && a.side == b.side;
}

// scan_kernel<nt, k8, its, debug>; nt == 0: no form
struct Scan16Form {
    int nt;
    bool k8;
    int its;
    bool debug;
};
inline bool operator==(const Scan16Form& a, const Scan16Form& b) { return a.nt == b.nt && a.k8 == b.k8 && a.its == b.its && a.debug == b.debug; }

// what one narrow-counter launch asks for
struct Scan8Ask {
    int kmax, kmin;                 // highest and lowest order
    int bits;                       // counter width, 4 or 8
    bool small_w;                   // windows of at most 2048 bases (else of at most 5120)
    bool debug;                     // the debug dump
    bool sample;                    // the sample of the adaptive width
    bool side;                      // the side table for the period-4 max-mers
    bool kmin1_form;                // ScanSchedule::kmin1_form: a 4-bit bulk launch takes the form compiled for the lowest order 1
    bool slides;                    // the schedule's windows slide (slide_pp > 0) ...
    bool listed;                    // ... but not those of a launch that walks a hand-over list
};

// The form of one narrow-counter launch.  No form where the kernels have none for the request: the sample and the side table exist
// for 4-bit counters at K = 8, without the debug dump and over a range; K = 6 and 7 have 8-bit counters only.  kmin1_form is a
// statement about the scan, not about the launch: a launch that has no such form (another width, a hand-over list) keeps its own.
inline Scan8Form scan8_form_of(const Scan8Ask& a) {
    const Scan8Form none = {0, 0, 0, 0, false, 0, false};
    const int its = a.small_w ? 8 : 20;
    const int no_slide = (a.slides && !a.listed) ? 0 : SCAN8_ROLE_NO_SLIDE;
    const bool plain4 = a.kmax == 8 && a.bits == 4 && !a.debug && !a.listed;        // where the sample and the side table exist
    if (a.sample) return plain4 ? Scan8Form{8, its, 4, 3, false, SCAN8_ROLE_SAMPLE | no_slide, true} : none;
    if (a.side && !plain4) return none;
    if (a.kmax == 6 || a.kmax == 7)     // the 8-bit table is 16 / 4 KiB - registers, not LDS, bound the workgroups per CU
        return a.bits == 8 ? Scan8Form{a.kmax, its, 8, FRISK_K7_WPS, a.debug, 0, false} : none;
    if (a.kmax != 8) return none;
    if (a.bits == 8) return Scan8Form{8, its, 8, 2, a.debug, 0, false};
    if (a.bits != 4) return none;
    if (a.debug) return Scan8Form{8, its, 4, 3, true, 0, false};        // (with the ring, sliding or not)
    const int kmin1 = (a.kmin1_form && !a.listed && a.kmin == 1) ? SCAN8_ROLE_KMIN1 : 0;
    return Scan8Form{8, its, 4, 3, false, kmin1 | no_slide, a.side};
}

// The form of scan_kernel.h's launch: one 512-thread workgroup per CU with the per-position loops unrolled its = 4 / 10 / 16 times,
// or 1024 threads and runtime loops (its = 0); the debug dump exists for the longest unrolled class and for the runtime loops.
// two_wg: two 256-thread workgroups per CU (K <= 7, no debug dump), its = 8 or 20.
inline Scan16Form scan16_form_of(int kmax, int its, bool debug, bool two_wg) {
    const Scan16Form none = {0, false, 0, false};
    if (kmax > 8) return none;
    if (two_wg) return (kmax <= 7 && !debug && (its == 8 || its == 20)) ? Scan16Form{256, false, its, false} : none;
    const bool k8 = kmax == 8;
    if (debug) return its ? Scan16Form{512, k8, 16, true} : Scan16Form{1024, k8, 0, true};
    if (its == 4 || its == 10 || its == 16) return Scan16Form{512, k8, its, false};
    return its == 0 ? Scan16Form{1024, k8, 0, false} : none;
}

// Every instantiation of scan8_kernel, as X(KMAX, ITS, BITS, WPS, DEBUG, ROLE, SIDE), in the sub-lists by which the units instantiate
// them (the cut exists for build time alone).
// K = 8 with 4-bit counters and the lowest order an argument (scan8_launch4.hip): the sample and the side-table form, each sliding or
// not, then the plain form - debug, not sliding, sliding
#define FRISK_SCAN8_4BIT_GENERIC_FORMS(X)                                                                       \
    X(8, 8, 4, 3, false, SCAN8_ROLE_SAMPLE, true) X(8, 8, 4, 3, false, SCAN8_ROLE_SAMPLE | SCAN8_ROLE_NO_SLIDE, true)       \
    X(8, 20, 4, 3, false, SCAN8_ROLE_SAMPLE, true) X(8, 20, 4, 3, false, SCAN8_ROLE_SAMPLE | SCAN8_ROLE_NO_SLIDE, true)     \
    X(8, 8, 4, 3, false, 0, true) X(8, 8, 4, 3, false, SCAN8_ROLE_NO_SLIDE, true)                               \
    X(8, 20, 4, 3, false, 0, true) X(8, 20, 4, 3, false, SCAN8_ROLE_NO_SLIDE, true)                             \
    X(8, 8, 4, 3, true, 0, false) X(8, 20, 4, 3, true, 0, false)                                                \
    X(8, 8, 4, 3, false, SCAN8_ROLE_NO_SLIDE, false) X(8, 20, 4, 3, false, SCAN8_ROLE_NO_SLIDE, false)          \
    X(8, 8, 4, 3, false, 0, false) X(8, 20, 4, 3, false, 0, false)
// the 4-bit bulk forms again with the lowest order fixed at 1 (scan8_launch41.hip)
#define FRISK_SCAN8_4BIT_KMIN1_FORMS(X)                                                                         \
    X(8, 8, 4, 3, false, SCAN8_ROLE_KMIN1, true) X(8, 8, 4, 3, false, SCAN8_ROLE_KMIN1 | SCAN8_ROLE_NO_SLIDE, true)         \
    X(8, 20, 4, 3, false, SCAN8_ROLE_KMIN1, true) X(8, 20, 4, 3, false, SCAN8_ROLE_KMIN1 | SCAN8_ROLE_NO_SLIDE, true)       \
    X(8, 8, 4, 3, false, SCAN8_ROLE_KMIN1 | SCAN8_ROLE_NO_SLIDE, false) X(8, 20, 4, 3, false, SCAN8_ROLE_KMIN1 | SCAN8_ROLE_NO_SLIDE, false) \
    X(8, 8, 4, 3, false, SCAN8_ROLE_KMIN1, false) X(8, 20, 4, 3, false, SCAN8_ROLE_KMIN1, false)
// 8-bit counters: K = 8, and K = 7 and 6 (scan8_launch.hip)
#define FRISK_SCAN8_8BIT_FORMS(X)                                                                               \
    X(8, 8, 8, 2, false, 0, false) X(8, 20, 8, 2, false, 0, false) X(8, 8, 8, 2, true, 0, false) X(8, 20, 8, 2, true, 0, false)     \
    X(7, 8, 8, FRISK_K7_WPS, false, 0, false) X(7, 20, 8, FRISK_K7_WPS, false, 0, false)                        \
    X(7, 8, 8, FRISK_K7_WPS, true, 0, false) X(7, 20, 8, FRISK_K7_WPS, true, 0, false)                          \
    X(6, 8, 8, FRISK_K7_WPS, false, 0, false) X(6, 20, 8, FRISK_K7_WPS, false, 0, false)                        \
    X(6, 8, 8, FRISK_K7_WPS, true, 0, false) X(6, 20, 8, FRISK_K7_WPS, true, 0, false)
#define FRISK_SCAN8_FORMS(X) FRISK_SCAN8_4BIT_GENERIC_FORMS(X) FRISK_SCAN8_4BIT_KMIN1_FORMS(X) FRISK_SCAN8_8BIT_FORMS(X)

// every instantiation of scan_kernel, as X(NT, K8, ITS, DEBUG): by window class with and without the order-8 table, then the two
// workgroups per CU
#define FRISK_SCAN16_FORMS(X)                                                                                   \
    X(512, true, 4, false) X(512, true, 10, false) X(512, true, 16, false) X(1024, true, 0, false)              \
    X(512, true, 16, true) X(1024, true, 0, true)                                                               \
    X(512, false, 4, false) X(512, false, 10, false) X(512, false, 16, false) X(1024, false, 0, false)          \
    X(512, false, 16, true) X(1024, false, 0, true)                                                             \
    X(256, false, 8, false) X(256, false, 20, false)
