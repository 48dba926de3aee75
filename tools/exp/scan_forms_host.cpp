// (CPU) which instantiation of the scan kernels every launch of a scan runs: plan_scan_schedule's statements ScanSchedule::form_* and
// form16 (scan_schedule.h, scan_forms.h) over the shapes of scan_dispatch_host.cpp - lowest order 1..5, highest order 6..8, both
// counter widths, the side table and the adaptive choice, each with and without the debug dump, windows of both classes and one beyond
// the narrow-counter kernels, sliding and not - and over shapes off the narrow-counter path (every window class of scan_kernel.h, one
// and two workgroups per CU).  Required: every launch that the enqueuer makes has a form; every form is a row of its family's table
// (FRISK_SCAN8_FORMS, FRISK_SCAN16_FORMS); every form is what the rule - restated below, one clause per launch kind - says; the kmin = 1
// role sits on the 4-bit bulk forms of the schedules that name it and nowhere else.  With a file of the former launcher's answers
// (tests/golden/scan8_dispatch_parent.tsv: one narrow-counter request per line and the instantiation it launched) as argument:
// scan8_form_of gives every request the same form or none, and none to no request that a schedule of the sweep makes.
// Build: c++ -std=c++17 -O1 [-fsanitize=address,undefined] -Ifrisk_amd/csrc tools/exp/scan_forms_host.cpp -o scan_forms_host
#include <cstdio>
#include <cstring>

#include "scan_schedule.h"

static long fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++fails <= 20) {                                             \
                std::fprintf(stderr, "scan_forms_host: %s failed: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);                           \
                std::fprintf(stderr, "\n");                                  \
            }                                                                \
        }                                                                    \
    } while (0)

// an upper bound of scan_kernel.h's LDS (make_layout at kmin = 1): the decisions under test do not read it below 160 KB
static uint32_t lds_of(int K, int64_t maxwin, int lv) {
    int64_t bins = 0;
    for (int k = 1; k <= (K == 8 ? 6 : K); ++k) bins += int64_t(1) << (2 * k);
    int64_t o = (K == 8 ? 131072 : 0) + (bins * 2 + 15) / 16 * 16;
    if (K == 8) o += (scan_orphan_cap(maxwin) * 2 + 15) / 16 * 16;
    if (lv) o += 1024 * 8 + 1024 * 4;
    return uint32_t(o + 16 * 8 + 128 * 16 + (2 * 16 * 4 + 16 * 6 * 8));
}

// the tables, as arrays
#define ROW8(K_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_) {K_, ITS_, BITS_, WPS_, DBG_, ROLE_, SIDE_},
static const Scan8Form table8[] = {FRISK_SCAN8_FORMS(ROW8)};
#undef ROW8
#define ROW16(NT_, K8_, ITS_, DBG_) {NT_, K8_, ITS_, DBG_},
static const Scan16Form table16[] = {FRISK_SCAN16_FORMS(ROW16)};
#undef ROW16
static const int N8 = int(sizeof(table8) / sizeof(table8[0])), N16 = int(sizeof(table16) / sizeof(table16[0]));
static bool reached8[64], reached16[32];

static bool is_none(const Scan8Form& f) { return f.kmax == 0; }
static bool is_none(const Scan16Form& f) { return f.nt == 0; }
static int row_of(const Scan8Form& f) { for (int i = 0; i < N8; ++i) if (table8[i] == f) return i; return -1; }
static int row_of(const Scan16Form& f) { for (int i = 0; i < N16; ++i) if (table16[i] == f) return i; return -1; }

// a narrow-counter request as the fixture keys it (the rule reads of the lowest order only whether it is 1)
static bool made[3 * 512];
static int key_of(int kmax, int bits, bool small_w, bool debug, bool sample, bool side, bool kmin1, bool slides, bool listed, int kmin) {
    return ((((((((((kmax - 6) * 2 + (bits == 8)) * 2 + small_w) * 2 + debug) * 2 + sample) * 2 + side) * 2 + kmin1) * 2 + slides) * 2 + listed) * 2) + (kmin == 1 ? 0 : 1);
}

static long launches = 0, kmin1_launches = 0;

// one narrow-counter launch of a schedule: it has a form, the form is a row, and it is `want`
static void narrow_launch(const char* what, const ScanShape& s, const Scan8Form& got, const Scan8Form& want) {
    ++launches;
    CHECK(!is_none(got), "%s: no form (kmin %d K %d n %ld w %d inc %d flags %u debug %d)", what, s.kmin, s.kmax, long(s.n), s.w, s.inc, s.flags, int(s.debug));
    const int row = row_of(got);
    CHECK(row >= 0, "%s: <%d, %d, %d, %d, %d, %d, %d> is no row of FRISK_SCAN8_FORMS", what, got.kmax, got.its, got.bits, got.wps, int(got.debug), got.role, int(got.side));
    if (row >= 0) reached8[row] = true;
    CHECK(got == want, "%s: <%d, %d, %d, %d, %d, %d, %d>, the rule says <%d, %d, %d, %d, %d, %d, %d> (kmin %d K %d n %ld w %d inc %d flags %u debug %d)", what,
          got.kmax, got.its, got.bits, got.wps, int(got.debug), got.role, int(got.side), want.kmax, want.its, want.bits, want.wps, int(want.debug), want.role,
          int(want.side), s.kmin, s.kmax, long(s.n), s.w, s.inc, s.flags, int(s.debug));
    if (got.role & SCAN8_ROLE_KMIN1) ++kmin1_launches;
}

static void check_schedule(const ScanShape& s) {
    const ScanSchedule S = plan_scan_schedule(s);
    CHECK(S.error == nullptr, "kmin %d K %d n %ld w %d inc %d flags %u", s.kmin, s.kmax, long(s.n), s.w, s.inc, s.flags);
    if (S.error) return;
    const int K = s.kmax;
    const bool debug = s.debug;
    // the 16-bit family: the whole range off the narrow-counter path, list 2 on it; the long-window kernel is no form of it
    if (S.path == SCAN_PATH_BIG) {
        CHECK(is_none(S.form16), "the long-window path launches no 16-bit form");
    } else {
        const int need = int((s.plan_maxwin + 511) / 512);
        Scan16Form want;
        if (S.path == SCAN_PATH_TWO_WG) want = Scan16Form{256, false, s.plan_maxwin <= 2048 ? 8 : 20, false};
        else if (debug) want = need <= 16 ? Scan16Form{512, K == 8, 16, true} : Scan16Form{1024, K == 8, 0, true};
        else want = need <= 4 ? Scan16Form{512, K == 8, 4, false} : need <= 10 ? Scan16Form{512, K == 8, 10, false}
                  : need <= 16 ? Scan16Form{512, K == 8, 16, false} : Scan16Form{1024, K == 8, 0, false};
        CHECK(!is_none(S.form16), "no 16-bit form (K %d w %d debug %d)", K, s.w, int(debug));
        const int row = row_of(S.form16);
        CHECK(row >= 0, "<%d, %d, %d, %d> is no row of FRISK_SCAN16_FORMS", S.form16.nt, int(S.form16.k8), S.form16.its, int(S.form16.debug));
        if (row >= 0) reached16[row] = true;
        CHECK(S.form16 == want, "<%d, %d, %d, %d>, the rule says <%d, %d, %d, %d> (K %d w %d debug %d path %d)", S.form16.nt, int(S.form16.k8), S.form16.its,
              int(S.form16.debug), want.nt, int(want.k8), want.its, int(want.debug), K, s.w, int(debug), int(S.path));
    }
    if (S.path != SCAN_PATH_NARROW) {
        CHECK(is_none(S.form_sample) && is_none(S.form_bulk) && is_none(S.form_verdict[0]) && is_none(S.form_verdict[1]) && is_none(S.form_verdict[2]) &&
              is_none(S.form_handover), "a narrow-counter form off the narrow-counter path");
        return;
    }
    // the narrow-counter family.  ITS by window class; a range launch slides where the schedule does, a launch over a list never
    const int its = s.w <= 2048 ? 8 : 20;
    const int no_slide = S.slide_pp > 0 ? 0 : SCAN8_ROLE_NO_SLIDE;
    const int kmin1 = S.kmin1_form ? SCAN8_ROLE_KMIN1 : 0;
    const bool sw = s.w <= 2048, slides = S.slide_pp > 0;
    const long kmin1_before = kmin1_launches;
    long kmin1_wanted = 0;
    if (S.sample) {
        CHECK(K == 8 && !debug, "the sample is taken at K = 8 without the debug dump");
        // where the sample: 4-bit counters and the side table, a role of its own
        narrow_launch("sample", s, S.form_sample, Scan8Form{8, its, 4, 3, false, SCAN8_ROLE_SAMPLE | no_slide, true});
        // where the three bulk launches behind the verdict: plain 4-bit, 4-bit + side table (both with the scan's kmin = 1 statement), 8-bit
        narrow_launch("verdict 1", s, S.form_verdict[0], Scan8Form{8, its, 4, 3, false, kmin1 | no_slide, false});
        narrow_launch("verdict 2", s, S.form_verdict[1], Scan8Form{8, its, 4, 3, false, kmin1 | no_slide, true});
        narrow_launch("verdict 3", s, S.form_verdict[2], Scan8Form{8, its, 8, 2, false, 0, false});
        CHECK(is_none(S.form_bulk), "a sampled scan has the three launches behind the verdict, no fourth");
        kmin1_wanted = S.kmin1_form ? 2 : 0;
        for (int k1 = 0; k1 < 2; ++k1) {        // (as the schedule states its requests, and as the former enqueuer did)
            made[key_of(8, 4, sw, false, true, false, k1 && S.kmin1_form, slides, false, s.kmin)] = true;
            made[key_of(8, 8, sw, false, false, false, k1 && S.kmin1_form, slides, false, s.kmin)] = true;
        }
        made[key_of(8, 4, sw, false, false, false, S.kmin1_form, slides, false, s.kmin)] = true;
        made[key_of(8, 4, sw, false, false, true, S.kmin1_form, slides, false, s.kmin)] = true;
    } else {
        CHECK(is_none(S.form_sample) && is_none(S.form_verdict[0]) && is_none(S.form_verdict[1]) && is_none(S.form_verdict[2]), "forms of a sample that is not taken");
        Scan8Form want;
        // where K = 7 and 6: 8-bit counters, four workgroups per CU
        if (K == 7 || K == 6) { CHECK(S.bulk == 8 && !S.side, "K = 6, 7 count in 8 bits"); want = Scan8Form{K, its, 8, FRISK_K7_WPS, debug, 0, false}; }
        // where the 8-bit bulk at K = 8
        else if (S.bulk == 8) { CHECK(!S.side, "the side table belongs to 4-bit counters"); want = Scan8Form{8, its, 8, 2, debug, 0, false}; }
        // where the 4-bit bulk with the debug dump: the one debug instantiation (no side table, no role)
        else if (debug) { CHECK(S.bulk == 4 && !S.side && !S.kmin1_form, "no side table and no kmin = 1 form under the debug dump"); want = Scan8Form{8, its, 4, 3, true, 0, false}; }
        // where the 4-bit bulk: plain or side table as the schedule says, compiled for kmin = 1 where the schedule says
        else { CHECK(S.bulk == 4, "a bulk of 4 or 8 bits"); want = Scan8Form{8, its, 4, 3, false, kmin1 | no_slide, S.side}; kmin1_wanted = S.kmin1_form ? 1 : 0; }
        narrow_launch("bulk", s, S.form_bulk, want);
        made[key_of(K, S.bulk, sw, debug, false, S.side, S.kmin1_form, slides, false, s.kmin)] = true;
    }
    if (S.sample || S.bulk == 4) {
        // where the hand-over of list 1: 8-bit counters at K = 8, over a list - no sliding, no role
        narrow_launch("hand-over", s, S.form_handover, Scan8Form{8, its, 8, 2, debug, 0, false});
        for (int k1 = 0; k1 < 2; ++k1) made[key_of(8, 8, sw, debug, false, false, k1 && S.kmin1_form, slides, true, s.kmin)] = true;
    } else {
        CHECK(is_none(S.form_handover), "an 8-bit bulk fills list 2: no launch over list 1");
    }
    // the kmin = 1 role: on the 4-bit bulk forms of a schedule that names it (above), on no other launch of that schedule, in no other schedule
    CHECK(kmin1_launches - kmin1_before == kmin1_wanted, "%ld launches with the kmin = 1 role, %ld 4-bit bulk launches of a schedule with kmin1_form %d",
          kmin1_launches - kmin1_before, kmin1_wanted, int(S.kmin1_form));
}

// the former launcher's answers: every request gets the same form or none, and none only where no schedule above asks
static void check_fixture(const char* path, long* same, long* none_unasked) {
    std::FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr, "cannot read %s", path);
    if (!f) return;
    char line[512];
    long requests = 0;
    while (std::fgets(line, sizeof(line), f)) {
        int v[17];
        if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10,
                        v + 11, v + 12, v + 13, v + 14, v + 15, v + 16) != 17) continue;         // (the two header lines)
        ++requests;
        Scan8Ask a = Scan8Ask();
        a.kmax = v[0]; a.bits = v[1]; a.small_w = v[2] != 0; a.debug = v[3] != 0; a.sample = v[4] != 0; a.side = v[5] != 0; a.kmin1_form = v[6] != 0;
        a.slides = v[7] != 0; a.listed = v[8] != 0; a.kmin = v[9];
        const Scan8Form was = {v[10], v[11], v[12], v[13], v[14] != 0, v[15], v[16] != 0};
        const Scan8Form got = scan8_form_of(a);
        CHECK(row_of(was) >= 0, "the former answer to request %ld is no row of the table", requests);
        if (is_none(got)) {
            CHECK(!made[key_of(a.kmax, a.bits, a.small_w, a.debug, a.sample, a.side, a.kmin1_form, a.slides, a.listed, a.kmin)],
                  "no form for a request that a schedule makes: %s", line);
            ++*none_unasked;
        } else {
            CHECK(got == was, "<%d, %d, %d, %d, %d, %d, %d> for %s", got.kmax, got.its, got.bits, got.wps, int(got.debug), got.role, int(got.side), line);
            ++*same;
        }
    }
    std::fclose(f);
    CHECK(requests == 3 * 2 * 2 * 2 * 2 * 2 * 2 * 2 * 2 * 2, "%ld requests in %s", requests, path);
}

int main(int argc, char** argv) {
    CHECK(N8 == 34 && N16 == 14, "%d + %d rows", N8, N16);
    for (int i = 0; i < N8; ++i) for (int j = 0; j < i; ++j) CHECK(!(table8[i] == table8[j]), "rows %d and %d of FRISK_SCAN8_FORMS are one instantiation", j, i);
    for (int i = 0; i < N16; ++i) for (int j = 0; j < i; ++j) CHECK(!(table16[i] == table16[j]), "rows %d and %d of FRISK_SCAN16_FORMS are one instantiation", j, i);
    long plans = 0;
    // scan_dispatch_host.cpp's shapes (FRISK_SCAN_SIDE4 with the debug dump and an increment above half a window for every width among them)
    const uint32_t widths[] = {0u, FRISK_SCAN_BITS4, FRISK_SCAN_SIDE4};
    const int hints[][2] = {{0, 0}, {4, 0}, {4, 1}, {8, 0}};
    const int64_t ns[] = {1, 43, 12063, 410000, 3058000};
    for (int kmin = 1; kmin <= 5; ++kmin) for (int K = 6; K <= 8; ++K) for (int64_t n : ns) for (int w : {2048, 5000, 5121})
    for (int inc : {w / 5, w / 2 + 1}) for (uint32_t width : widths) for (const auto& h : hints)
    for (uint32_t chunks : {0u, uint32_t(FRISK_SCAN_CHUNKS)}) for (int debug = 0; debug < 2; ++debug) for (int generic = 0; generic < 2; ++generic) {
        ScanShape s = ScanShape();
        s.kmin = kmin; s.kmax = K; s.num_cu = 256; s.n = n; s.w = w; s.inc = inc; s.plan_maxwin = w; s.debug = debug != 0;
        s.flags = width | chunks | (generic ? FRISK_SCAN_GENERIC : 0u);
        s.width_hint = h[0]; s.hint_side = h[1]; s.hint_matches = true;
        s.lv_shared = kmin <= 5 ? 5 : 0;
        s.lds_shared = lds_of(K, w, s.lv_shared); s.lds_level0 = lds_of(K, w, 0);
        check_schedule(s);
        ++plans;
    }
    // off the narrow-counter path: scan_kernel.h's window classes (4 / 10 / 16 unrolled positions per thread, runtime loops), one and two
    // workgroups per CU, the IVOM dump; the fixed 8-bit width on the path; orders and windows beyond the LDS kernels
    for (int K = 6; K <= 9; ++K) for (int w : {2048, 5000, 8000, 9000, 70000}) for (int debug = 0; debug < 2; ++debug) for (int variant = 0; variant < 4; ++variant) {
        ScanShape s = ScanShape();
        s.kmin = 1; s.kmax = K; s.num_cu = 256; s.n = 12063; s.w = w; s.inc = w / 5; s.plan_maxwin = w; s.debug = debug != 0;
        s.lv_shared = K >= 6 ? 5 : 0;
        s.lds_shared = lds_of(K, w, s.lv_shared); s.lds_level0 = lds_of(K, w, 0);
        if (variant == 0) { s.has_k8_bits = true; s.k8_bits = 16; }
        if (variant == 1) { s.has_k8_bits = true; s.k8_bits = 16; s.one_wg = true; }
        if (variant == 2) s.want_ivom = true;
        if (variant == 3) { s.has_k8_bits = true; s.k8_bits = 8; }
        check_schedule(s);
        ++plans;
    }
    long same = 0, none_unasked = 0;
    if (argc > 1) check_fixture(argv[1], &same, &none_unasked);
    int r8 = 0, r16 = 0;
    for (int i = 0; i < N8; ++i) r8 += reached8[i];
    for (int i = 0; i < N16; ++i) r16 += reached16[i];
    for (int i = 0; i < N8; ++i)
        if (!reached8[i]) std::printf("scan_forms_host: no schedule of the sweep reaches <%d, 256, %d, %d, 64, %d, %d, %d, %d>\n", table8[i].kmax, table8[i].its,
                                      table8[i].bits, table8[i].wps, int(table8[i].debug), table8[i].role, int(table8[i].side));
    for (int i = 0; i < N16; ++i)
        if (!reached16[i]) std::printf("scan_forms_host: no schedule of the sweep reaches scan_kernel<%d, %d, %d, %d>\n", table16[i].nt, int(table16[i].k8),
                                       table16[i].its, int(table16[i].debug));
    CHECK(launches > 0 && kmin1_launches > 0 && kmin1_launches < launches, "the sweep reaches launches with and without the kmin = 1 role");
    if (fails) { std::fprintf(stderr, "scan_forms_host: %ld checks failed\n", fails); return 1; }
    std::printf("scan_forms_host ok: %ld schedules, %ld narrow-counter launches (%ld with the kmin = 1 role), %d of %d + %d of %d rows reached; "
                "fixture: %ld requests keep their form, %ld that no schedule makes have none\n", plans, launches, kmin1_launches, r8, N8, r16, N16, same, none_unasked);
    return 0;
}
