// (CPU) the library's host-only headers under AddressSanitizer + UBSan (GPU sanitizers are not available on the pool): random batches
// through the 2-bit packer (against a letter-by-letter restatement), bitmap -> runs, the HMM fit / Viterbi on random series of awkward
// lengths, the scan's launch schedule (scan_schedule.h): invariants over a sweep of shapes, named shapes against values worked out by
// hand, the window-tile planner (scan_tiles.h): every rank's tiles of random shapes together, the region scorer's plan
// (range_plan.h): invariants over seeded random batches, named cases, the refusals with their rows, and the memory fit, the boundary
// refinement's plan (plan_refine: the cores and the search geometry over seeded random batches, named cases, every refusal) and its
// integer arithmetic (refine_math.h: flog2 against long double, the workgroup's change-point search against a scan), and phase A's
// plan (profile_plan.h): the launch of every form over a sweep of ranges, two named shapes, and the pieces of a streamed batch.
// build + run:  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifrisk_amd/csrc
//               tools/exp/san_host.cpp -o build/san/san_host -lpthread -lz && build/san/san_host
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include "seq_pack2.h"
#include "hmm_host.h"
#include "fasta_index.h"
#include "fasta_pack2.h"
#include "scan_schedule.h"
#include "scan_tiles.h"
#include "range_plan.h"
#include "refine_math.h"
#include "profile_plan.h"
#include <fstream>
#include <unistd.h>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// make_layout(1, K, scan_orphan_cap(maxwin), lv).total restated (scan_kernel.h is a HIP header): order-8 table, 16-bit tables of the
// orders 1..min(K, 6) or 1..K, orphan list (K = 8), prefix tables of level 5, window constants + log table + counters and scratch
static uint32_t lds_of(int K, int64_t maxwin, int lv) {
    int64_t bins = 0;
    for (int k = 1; k <= (K == 8 ? 6 : K); ++k) bins += int64_t(1) << (2 * k);
    int64_t o = (K == 8 ? 131072 : 0) + (bins * 2 + 15) / 16 * 16;
    if (K == 8) o += (scan_orphan_cap(maxwin) * 2 + 15) / 16 * 16;
    if (lv) o += 1024 * 8 + 1024 * 4;
    return uint32_t(o + 16 * 8 + 128 * 16 + (2 * 16 * 4 + 16 * 6 * 8));
}
static ScanShape shape_of(int K, int num_cu, int64_t n, int w, int inc, uint32_t flags = 0, int hint = 0, int hint_side = 0, bool debug = false) {
    ScanShape s = ScanShape();
    s.kmin = 1; s.kmax = K; s.num_cu = num_cu; s.n = n; s.w = w; s.inc = inc; s.flags = flags; s.plan_maxwin = w; s.debug = debug;
    s.rip = (flags & FRISK_SCAN_RIP) != 0;
    s.width_hint = hint; s.hint_side = hint_side; s.hint_matches = true;
    s.lv_shared = K >= 6 ? 5 : 0;
    s.lds_shared = lds_of(K, w, s.lv_shared); s.lds_level0 = lds_of(K, w, 0);
    return s;
}

static long long check_scan_schedule() {          // -> schedules planned
    const int64_t two17 = int64_t(1) << 17;
    // (a) invariants over a sweep
    const int64_t ns[] = {1, 2, 7, 8, 9, 40, 200, 767, 3000, 12063, 24575, 24576, 24577, two17 - 1, two17, two17 + 1, 386173, 1000000, 3058000, 4000000};
    const uint32_t flag_sets[] = {0u, FRISK_SCAN_CHUNKS, FRISK_SCAN_BITS4, FRISK_SCAN_SIDE4, FRISK_SCAN_CHUNKS | FRISK_SCAN_SIDE4 | FRISK_SCAN_RIP};
    const int hints[][2] = {{0, 0}, {4, 0}, {4, 1}, {8, 0}};
    int64_t plans = 0, two_segments = 0, sampled = 0;
    for (int64_t n : ns) for (int num_cu : {1, 8, 256}) for (int K : {4, 6, 7, 8, 9}) for (int w : {400, 2048, 2049, 5000, 5120, 5121}) {
        const int edge = (w - (K - 1)) / 2;                     // the largest inc with 2 inc <= w - (K - 1)
        for (int inc : {1, w / 4, edge - 1, edge, edge + 1, w / 2, w / 2 + 1, w}) for (uint32_t flags : flag_sets) for (const auto& h : hints) for (int debug = 0; debug < 2; ++debug) {
            ScanShape s = shape_of(K, num_cu, n, w, inc, flags, h[0], h[1], debug != 0);
            const ScanSchedule S = plan_scan_schedule(s);
            ++plans;
            CHECK(S.error == nullptr);
            if (S.error) continue;
            CHECK(S.grid >= 1 && (S.grid < 8 || S.grid % 8 == 0));
            CHECK(S.packed_rows == (n < two17));
            CHECK(S.chunk >= 1 && S.orphan_cap == w / 8 + 2 && S.lds_total <= 160u * 1024 + (K > 8 ? ~0u / 2 : 0u));
            CHECK((S.segments == 2) == (0 < S.cut && S.cut < n) && (S.segments == 1 || S.segments == 2) && (S.segments == 2 || S.cut == n));
            CHECK((S.path == SCAN_PATH_BIG) == (K > 8) && S.big_grid == (K > 8 ? int(std::min<int64_t>(n, num_cu)) : 0));
            if (S.packed_rows) {
                const RowBlock& b = S.block;
                const size_t N = size_t(n), cols[] = {b.start, b.stop, b.kld, b.gc};
                for (int i = 0; i < 4; ++i) CHECK(cols[i] == (i ? cols[i - 1] + (N + 1) / 2 * 2 : 0) && cols[i] + N <= (i < 3 ? cols[i + 1] : s.rip ? b.pi : b.seq_index));
                if (s.rip) CHECK(b.gc + N <= b.pi && b.pi + N <= b.si && b.si + N <= b.cri && b.cri + N <= b.seq_index);
                // (offsets are in 8-byte words: the two 4-byte columns start on a multiple of 8 bytes and do not meet)
                CHECK(b.seq_index * 8 + N * 4 <= b.status * 8 && b.status * 8 + N * 4 <= b.words * 8);
            }
            if (S.path != SCAN_PATH_NARROW) {
                CHECK(!S.sample && !S.side && S.ring_slices == 0 && S.slide_pp == 0 && S.segments == 1 && S.bulk == 16);
                continue;
            }
            CHECK((K == 8 && w <= 5120 && S.narrow8) || ((K == 6 || K == 7) && w <= 5120 && !S.narrow8));
            CHECK(S.chunk8 >= 1 && S.nchunks == (n + S.chunk8 - 1) / S.chunk8);
            CHECK(S.can_slide == (2 * inc <= w - (K - 1)));
            CHECK(S.slide_pp == 0 || (S.can_slide && S.chunk8 >= 2));
            CHECK(!S.dealt || (S.chunk8 >= 4 && !S.short_scan));
            if (S.segments == 2) CHECK(S.cut % (S.chunk8 * S.sel_mod) == 0 && n >= two17 && !debug);
            CHECK(!S.sample || (S.nchunks >= 64 * S.sel_mod && !debug && h[0] == 0 && S.bulk == 4 && S.sel_mode == 2 && S.nsample == (S.nchunks + S.sel_mod - 1) / S.sel_mod));
            CHECK(S.sample || (S.sel_mode == 0 && S.nsample == 0));
            CHECK(!S.side || (S.narrow8 && S.bulk == 4 && !debug));
            CHECK(S.bulk == 4 || S.bulk == 8);
            CHECK(S.ring_slices == 0 || (S.narrow8 && (S.slide_pp > 0 || debug) && S.ring_slices <= 4 * int64_t(num_cu) && S.ring_slices <= S.nchunks));
            two_segments += S.segments == 2; sampled += S.sample;
        }
    }
    CHECK(two_segments > 1000 && sampled > 1000);              // (the sweep reaches both)
    // (b) named shapes: 256 CUs, K = 1..8, w = 5000, inc = 1000, no flags, no hint, not debug.  Every value below is worked out by hand
    // from the rules ("frisk_scan in five steps"; the measurements behind them are in NOTES.md)
    {   // BASELINE's C3: short (< 2 x 16 windows per workgroup of 768): two static rounds, ceil(12 063 / 1 536) = 8 windows per chunk
        const ScanSchedule S = plan_scan_schedule(shape_of(8, 256, 12063, 5000, 1000));
        CHECK(S.path == SCAN_PATH_NARROW && S.narrow8 && !S.small_w && S.chunk8 == 8 && S.short_scan && S.slide_pp == 4 && S.nchunks == 1508);
        CHECK(S.sel_mod == 16 && !S.dealt && S.sample && S.nsample == 95 && S.ring_slices == 1024 && S.cut == 12063 && S.segments == 1 && S.packed_rows);
        CHECK(S.lv == 5 && S.lds_total == 158624 && S.grid == 256 && S.its == 10 && S.orphan_cap == 627);
    }
    {   // the bench shard: chunks of 16, dealt; 24 136 chunks, every 32nd sampled; units of 512 windows, 754 whole ones: the tail first takes
        // 47 units (1 512 chunks), which is 2 rounds of 768 workgroups = 24 576 windows, and the cut rounds up to unit 707
        ScanShape s = shape_of(8, 256, 386173, 5000, 1000);
        ScanSchedule S = plan_scan_schedule(s);
        CHECK(S.chunk8 == 16 && !S.short_scan && S.slide_pp == 4 && S.nchunks == 24136 && S.sel_mod == 32 && S.dealt && S.sample && S.nsample == 755);
        CHECK(S.ring_slices == 1024 && S.cut == 361984 && S.segments == 2 && !S.packed_rows && S.bulk == 4 && S.sel_mode == 2);
        s.width_hint = 8;               // 8-bit bulk on 512 workgroups: 3 rounds, the same 24 576 windows
        S = plan_scan_schedule(s);
        CHECK(S.cut == 361984 && !S.sample && S.bulk == 8 && S.sel_mode == 0 && !S.side);
        s.hint_matches = false;         // a hint taken with another geometry does not count
        CHECK(plan_scan_schedule(s).sample);
    }
    {   // 2^17: the shortest scan in two segments - 256 units, the last 16 (512 chunks, less than a round) on the tail stream
        const ScanSchedule S = plan_scan_schedule(shape_of(8, 256, two17, 5000, 1000));
        CHECK(S.nchunks == 8192 && S.sel_mod == 32 && S.cut == 122880 && S.segments == 2 && !S.packed_rows);
        const ScanSchedule T = plan_scan_schedule(shape_of(8, 256, two17 - 1, 5000, 1000));
        CHECK(T.cut == two17 - 1 && T.segments == 1 && T.packed_rows);
    }
    {   // a long scan: 191 125 chunks, the sample one round of 768 workgroups (stride 249); units of 3 984, tail of 15 rounds
        const ScanSchedule S = plan_scan_schedule(shape_of(8, 256, 3058000, 5000, 1000));
        CHECK(S.chunk8 == 16 && S.nchunks == 191125 && S.sel_mod == 249 && S.nsample == 768 && S.cut == 2876448 && S.segments == 2);
    }
    {   // 40 windows: one per chunk, nothing slides, so no ring either
        const ScanSchedule S = plan_scan_schedule(shape_of(8, 256, 40, 5000, 1000));
        CHECK(S.chunk8 == 1 && S.short_scan && S.slide_pp == 0 && !S.sample && S.ring_slices == 0 && S.nchunks == 40 && S.grid == 40);
    }
    for (int inc : {2500, 2497}) {      // 2 inc > w - 7: not sliding, window by window; 3 000 chunks >= 64 x 32: stride 32, 94 sampled
        const ScanSchedule S = plan_scan_schedule(shape_of(8, 256, 3000, 5000, inc));
        CHECK(!S.can_slide && S.chunk8 == 1 && S.sel_mod == 32 && S.sample && S.nsample == 94 && S.slide_pp == 0 && S.ring_slices == 0);
    }
    CHECK(plan_scan_schedule(shape_of(8, 256, 3000, 5000, 2496)).can_slide);
    {   // FRISK_SCAN_CHUNKS: chunks of 8 dealt by counters whatever the size
        const ScanSchedule S = plan_scan_schedule(shape_of(8, 256, 200, 400, 150, FRISK_SCAN_CHUNKS));
        CHECK(S.small_w && S.chunk8 == 8 && S.dealt && !S.short_scan && S.slide_pp == 1 && !S.sample && S.nchunks == 25 && S.ring_slices == 25);
    }
    {   // the other paths, the LDS fall-back and the two refusals
        CHECK(plan_scan_schedule(shape_of(6, 256, 5000, 400, 150)).path == SCAN_PATH_NARROW);
        const ScanSchedule S4 = plan_scan_schedule(shape_of(4, 256, 5000, 400, 150));
        CHECK(S4.path == SCAN_PATH_TWO_WG && S4.grid == 512 && S4.chunk == 1 && S4.its == 8);
        CHECK(plan_scan_schedule(shape_of(4, 256, 5000, 400, 150, 0, 0, 0, true)).path == SCAN_PATH_16BIT);
        const ScanSchedule S8 = plan_scan_schedule(shape_of(8, 256, 5000, 5121, 1000));
        CHECK(S8.path == SCAN_PATH_16BIT && S8.its == 16 && S8.grid == 256 && S8.chunk == 2);
        ScanShape s = shape_of(8, 256, 5000, 5000, 1000);
        s.plan_maxwin = 60000; s.lds_shared = lds_of(8, 60000, 5); s.lds_level0 = lds_of(8, 60000, 0);       // a rescued scaffold of 60 kb
        ScanSchedule S = plan_scan_schedule(s);
        CHECK(s.lds_shared > 160u * 1024 && S.error == nullptr && S.lv == 0 && S.lds_total == s.lds_level0 && S.its == 0 && S.path == SCAN_PATH_NARROW);
        s.lds_level0 = 160 * 1024 + 16;
        S = plan_scan_schedule(s);
        CHECK(S.error && std::string(S.error) == "window too long for the 160 KB LDS of one workgroup" && S.error_code == FRISK_E_ARG);
        s.plan_maxwin = 65536;
        S = plan_scan_schedule(s);
        CHECK(S.error == nullptr && S.path == SCAN_PATH_BIG && S.big_grid == 256);
    }
    return (long long)plans;
}

// Window-tile sharding (scan_tiles.h): over seeded random shapes, every rank's plan_tiles() together.  The ranks' candidate ranges
// partition the job's numbering; every window is scored by exactly one rank and every base counted by exactly one; what a tile
// keeps resident, [base0, tile_end), holds its windows and its owned positions with the kmax - 1 bases behind them.
static long long check_scan_tiles() {             // -> shapes planned
    std::mt19937_64 rng(20240607);
    const int shapes = 20000;
    long long jumpbacks = 0, small_tiles = 0, windowless = 0, split_scaffolds = 0;
    for (int shape = 0; shape < shapes; ++shape) {
        const int32_t w = 1 + int32_t(rng() % 60), inc = 1 + int32_t(rng() % 40);
        const bool all = (rng() & 1) != 0;
        const int kmax = 1 + int(rng() % 12), world = 1 + int(rng() % 9);
        std::vector<int64_t> lens(size_t(rng() % 7));
        for (int64_t& n : lens) {
            switch (rng() % 4) {
                case 0: n = 0; break;
                case 1: n = int64_t(rng() % uint64_t(2 * w + 2)); break;
                case 2: n = std::max<int64_t>(0, int64_t(1.75 * w) - inc + int64_t(rng() % 5) - 2); break;      // the small-scaffold limit
                default: n = int64_t(rng() % 401); break;
            }
        }
        std::vector<int64_t> ncand(lens.size());
        std::vector<std::vector<int>> scored(lens.size()), counted(lens.size());       // per window, per base: by how many ranks
        std::vector<int> in_tiles(lens.size(), 0);
        int64_t total = 0;
        for (size_t s = 0; s < lens.size(); ++s) {
            int32_t kind = 0;
            plan_scaffold(lens[s], w, inc, all, ncand[s], kind);
            total += ncand[s];
            scored[s].assign(size_t(ncand[s]), 0);
            counted[s].assign(size_t(lens[s]), 0);
        }
        int64_t prev_c1 = 0;
        for (int rank = 0; rank < world; ++rank) {
            int64_t c0 = -1, c1 = -1;
            const std::vector<Tile> tiles = plan_tiles(lens, w, inc, all, kmax, rank, world, c0, c1);
            CHECK(c0 == prev_c1 && c0 <= c1 && c1 <= total);
            prev_c1 = c1;
            int64_t mine = 0;
            int32_t prev_scaf = -1;
            for (const Tile& t : tiles) {
                CHECK(t.scaf > prev_scaf && size_t(t.scaf) < lens.size());
                prev_scaf = t.scaf;
                if (t.scaf < 0 || size_t(t.scaf) >= lens.size()) continue;
                const size_t s = size_t(t.scaf);
                const int64_t size = lens[s], end = tile_end(t, w, inc, kmax);
                ++in_tiles[s];
                mine += t.ncand;
                CHECK(t.size == size && 0 <= t.base0 && t.base0 <= end && end <= size);
                CHECK(0 <= t.j0 && 0 <= t.ncand && t.j0 + t.ncand <= ncand[s]);
                CHECK(0 <= t.own0 && t.own0 <= t.own1 && t.own1 <= size);
                if (!(0 <= t.j0 && 0 <= t.ncand && t.j0 + t.ncand <= ncand[s] && 0 <= t.own0 && t.own0 <= t.own1 && t.own1 <= size)) continue;
                for (int64_t p = t.own0; p < t.own1; ++p) ++counted[s][size_t(p)];
                if (t.own1 > t.own0) CHECK(t.base0 <= t.own0 && std::min<int64_t>(size, t.own1 + kmax - 1) <= end);
                for (int64_t j = t.j0; j < t.j0 + t.ncand; ++j) {
                    ++scored[s][size_t(j)];
                    int64_t a = j * inc, b = a + w;
                    if (b > size) { a = std::max<int64_t>(0, size - w); b = size; ++jumpbacks; }       // the jumpback window
                    CHECK(t.base0 <= a && b <= end);
                }
                small_tiles += t.kind == 1; windowless += t.ncand == 0; split_scaffolds += t.ncand > 0 && t.ncand < ncand[s];
            }
            CHECK(mine == c1 - c0);
        }
        CHECK(prev_c1 == total);
        for (size_t s = 0; s < lens.size(); ++s) {
            for (int n : scored[s]) CHECK(n == 1);
            for (int n : counted[s]) CHECK(n == 1);
            if (lens[s] == 0) CHECK(in_tiles[s] <= 1);
        }
    }
    CHECK(jumpbacks > 1000 && small_tiles > 1000 && windowless > 1000 && split_scaffolds > 1000);      // (the sweep reaches them)
    return shapes;
}

// The region scorer's plan (range_plan.h).  Invariants of an accepted plan: the two lists partition the rows, each longest first with
// ties by row; a short row is at most FRISK_RANGE_SHORT_MAX bases; long_cap = n_long, plus n_short only at kmax = 8; the slice
// capacities are even and hold min(longest, 4^kmax); the grids follow the rules; the fit stays within 1 .. want.
static void check_one_plan(const RangePlan& R, const std::vector<int64_t>& seq_off, const std::vector<int32_t>& si, const std::vector<int64_t>& a,
                           const std::vector<int64_t>& b, int kmax, bool all_long, int num_cu, int per_cu, int top_n) {
    const int64_t n = int64_t(si.size());
    CHECK(R.error_code == FRISK_OK && R.error.empty());
    if (R.error_code != FRISK_OK) return;
    CHECK(int64_t(R.ranges.size()) == 2 * n && R.n_short() + R.n_long() == n);
    if (int64_t(R.ranges.size()) != 2 * n || R.n_short() + R.n_long() != n) return;
    std::vector<int> seen(static_cast<size_t>(n), 0);
    int64_t longest_short = 0, longest_long = 0;
    for (int form = 0; form < 2; ++form) {
        const std::vector<int64_t>& rows = form ? R.long_rows : R.short_rows;
        for (size_t i = 0; i < rows.size(); ++i) {
            const int64_t r = rows[i];
            CHECK(0 <= r && r < n);
            if (r < 0 || r >= n) return;
            ++seen[size_t(r)];
            const int64_t len = R.ranges[size_t(2 * r + 1)];
            CHECK(R.ranges[size_t(2 * r)] == seq_off[size_t(si[size_t(r)])] + a[size_t(r)] && len == b[size_t(r)] - a[size_t(r)] && len >= 1);
            CHECK((form == 1) == (all_long || len > FRISK_RANGE_SHORT_MAX));
            if (i > 0) {
                const int64_t p = rows[i - 1], plen = R.ranges[size_t(2 * p + 1)];
                CHECK(plen > len || (plen == len && p < r));
            }
            int64_t& longest = form ? longest_long : longest_short;
            longest = std::max(longest, len);
        }
    }
    for (int k : seen) CHECK(k == 1);
    const bool k8 = kmax == 8;
    CHECK(R.long_cap == R.n_long() + (k8 ? R.n_short() : 0));
    const int64_t nK = int64_t(1) << (2 * kmax);
    if (top_n > 0) {
        CHECK(R.cap_short % 2 == 0 && R.cap_short >= std::min(longest_short, nK) && R.cap_short <= std::min(longest_short, nK) + 1);
        const int64_t held = std::max(longest_long, k8 ? longest_short : 0);
        CHECK(R.cap_long % 2 == 0 && R.cap_long >= std::min(held, nK) && R.cap_long <= std::min(held, nK) + 1);
    } else {
        CHECK(R.cap_short == 0 && R.cap_long == 0);
    }
    CHECK(R.grid_short == int(std::min<int64_t>(R.n_short(), int64_t(num_cu) * (k8 ? 1 : per_cu))));
    CHECK(R.want_long <= num_cu && R.want_long <= R.long_cap && R.want_long >= std::min<int64_t>(R.n_long(), num_cu));
    CHECK((R.want_long == 0) == (R.long_cap == 0));
    if (R.want_long > 0) {
        const int64_t stride = (nK * 4 / 3 + 3) / 4 * 4;
        for (size_t slice : {size_t(0), size_t(R.cap_long) * 12}) for (size_t free_b : {size_t(0), size_t(1) << 20, size_t(1) << 34, size_t(1) << 40})
            for (size_t have : {size_t(0), size_t(stride), size_t(R.want_long) * size_t(stride)}) {
                const int64_t fit = fit_long_workgroups(R.want_long, stride, slice, free_b, have);
                CHECK(1 <= fit && fit <= R.want_long);
                if (free_b == (size_t(1) << 40)) CHECK(fit == R.want_long);
                if (free_b == 0 && slice == 0) CHECK(fit == std::max<int64_t>(1, std::min<int64_t>(R.want_long, int64_t(have / size_t(stride)))));
            }
    }
}

static long long check_range_plan() {             // -> plans made
    long long plans = 0;
    const int64_t two31 = int64_t(1) << 31;
    // (a) seeded random batches: scaffolds of up to 200 000 bases, lengths crowded at both sides of the short form's limit
    std::mt19937_64 rng(20240901);
    int64_t both_forms = 0, tied = 0;
    for (int round = 0; round < 3000; ++round) {
        const int n_seq = 1 + int(rng() % 5);
        std::vector<int64_t> seq_len(static_cast<size_t>(n_seq)), seq_off(static_cast<size_t>(n_seq));
        int64_t off = 0;
        for (int s = 0; s < n_seq; ++s) {
            seq_len[size_t(s)] = 1 + int64_t(rng() % 200000);
            seq_off[size_t(s)] = off;
            off += seq_len[size_t(s)] + 1;
        }
        const int64_t n = int64_t(rng() % 40);
        std::vector<int32_t> si(static_cast<size_t>(n));
        std::vector<int64_t> a(static_cast<size_t>(n)), b(static_cast<size_t>(n));
        for (int64_t r = 0; r < n; ++r) {
            const int32_t s = int32_t(rng() % uint64_t(n_seq));
            const int64_t size = seq_len[size_t(s)];
            int64_t len = 1 + int64_t(rng() % uint64_t(size));
            if (rng() % 3 == 0) len = std::min<int64_t>(size, 65533 + int64_t(rng() % 6));
            if (rng() % 4 == 0 && r > 0) len = std::min<int64_t>(size, b[size_t(r - 1)] - a[size_t(r - 1)]);       // a tie
            si[size_t(r)] = s;
            a[size_t(r)] = int64_t(rng() % uint64_t(size - len + 1));
            b[size_t(r)] = a[size_t(r)] + len;
        }
        const int kmax = 1 + int(rng() % 12), num_cu = 1 + int(rng() % 300), per_cu = (rng() & 1) ? 3 : 1;
        const bool all_long = kmax > 8 || rng() % 4 == 0;
        const int top_n = (rng() & 1) ? 1 + int(rng() % 64) : 0;
        const RangePlan R = plan_ranges(n_seq, seq_len.data(), seq_off.data(), si.data(), a.data(), b.data(), n, kmax, all_long, num_cu, per_cu, top_n);
        check_one_plan(R, seq_off, si, a, b, kmax, all_long, num_cu, per_cu, top_n);
        both_forms += R.n_short() > 0 && R.n_long() > 0;
        for (size_t i = 1; i < R.short_rows.size(); ++i) tied += R.ranges[size_t(2 * R.short_rows[i] + 1)] == R.ranges[size_t(2 * R.short_rows[i - 1] + 1)];
        ++plans;
    }
    CHECK(both_forms > 300 && tied > 300);                      // (the sweep reaches them)
    // (b) named cases on one batch: a scaffold of 2^31 + 10 bases behind one of 100 000 (no sequence is read)
    const std::vector<int64_t> seq_len = {100000, two31 + 10}, seq_off = {0, 100001};
    auto plan = [&](const std::vector<int32_t>& si, const std::vector<int64_t>& a, const std::vector<int64_t>& b, int kmax, bool all_long = false,
                    int top_n = 0, int per_cu = 3) {
        ++plans;
        return plan_ranges(2, seq_len.data(), seq_off.data(), si.data(), a.data(), b.data(), int64_t(si.size()), kmax, all_long, 256, per_cu, top_n);
    };
    {   // n = 0: an empty plan, nothing to launch
        const RangePlan R = plan({}, {}, {}, 8);
        check_one_plan(R, seq_off, {}, {}, {}, 8, false, 256, 3, 0);
        CHECK(R.grid_short == 0 && R.want_long == 0 && R.long_cap == 0);
    }
    for (int kmax : {8, 7, 9}) {        // a single row
        const RangePlan R = plan({0}, {5}, {505}, kmax, kmax > 8, 4);
        check_one_plan(R, seq_off, {0}, {5}, {505}, kmax, kmax > 8, 256, 3, 4);
        CHECK(R.ranges == (std::vector<int64_t>{5, 500}));
        if (kmax == 8) CHECK(R.n_short() == 1 && R.long_cap == 1 && R.grid_short == 1 && R.want_long == 1 && R.cap_short == 500 && R.cap_long == 500);
        if (kmax == 7) CHECK(R.n_short() == 1 && R.long_cap == 0 && R.grid_short == 1 && R.want_long == 0 && R.cap_short == 500 && R.cap_long == 0);
        if (kmax == 9) CHECK(R.n_long() == 1 && R.long_cap == 1 && R.grid_short == 0 && R.want_long == 1 && R.cap_short == 0 && R.cap_long == 500);
    }
    for (int kmax : {8, 7}) {           // 65 535 and 65 536 bases: either side of FRISK_RANGE_SHORT_MAX; 65 535 is odd, 4^7 = 16 384
        const std::vector<int32_t> si = {0, 0};
        const std::vector<int64_t> a = {10, 0}, b = {10 + 65535, 65536};
        const RangePlan R = plan(si, a, b, kmax, false, 64);
        check_one_plan(R, seq_off, si, a, b, kmax, false, 256, 3, 64);
        CHECK(R.short_rows == std::vector<int64_t>{0} && R.long_rows == std::vector<int64_t>{1});
        CHECK(R.long_cap == (kmax == 8 ? 2 : 1) && R.want_long == R.long_cap);
        CHECK(R.cap_short == (kmax == 8 ? 65536 : 16384) && R.cap_long == (kmax == 8 ? 65536 : 16384));
        const RangePlan B = plan(si, a, b, kmax, true);        // all_long: both rows to the long form, the longer first
        check_one_plan(B, seq_off, si, a, b, kmax, true, 256, 3, 0);
        CHECK(B.n_short() == 0 && B.long_rows == (std::vector<int64_t>{1, 0}) && B.long_cap == 2 && B.want_long == 2 && B.grid_short == 0);
    }
    {   // equal lengths: ties go by row, whatever the positions; 600 short rows on 256 CUs at three, or one, workgroups per CU
        std::vector<int32_t> si(600, 0);
        std::vector<int64_t> a(600), b(600);
        for (size_t r = 0; r < 600; ++r) { a[r] = int64_t(599 - r) * 7; b[r] = a[r] + (r % 3 == 0 ? 400 : 300); }
        for (int kmax : {7, 8}) for (int per_cu : {3, 1}) {
            const RangePlan R = plan(si, a, b, kmax, false, 0, per_cu);
            check_one_plan(R, seq_off, si, a, b, kmax, false, 256, per_cu, 0);
            CHECK(R.short_rows[0] == 0 && R.short_rows[1] == 3 && R.short_rows[199] == 597 && R.short_rows[200] == 1 && R.short_rows[201] == 2);
            CHECK(R.grid_short == (kmax == 8 || per_cu == 1 ? 256 : 600));
            CHECK(R.want_long == (kmax == 8 ? FRISK_RANGE_HANDOVER_WGS : 0) && R.long_cap == (kmax == 8 ? 600 : 0));
        }
    }
    {   // 2^31 - 1 bases are taken (the long form), 2^31 are refused, with the row
        const RangePlan R = plan({0, 1}, {0, 3}, {100, 3 + two31 - 1}, 8);
        check_one_plan(R, seq_off, {0, 1}, {0, 3}, {100, 3 + two31 - 1}, 8, false, 256, 3, 0);
        CHECK(R.long_rows == std::vector<int64_t>{1} && R.ranges[2] == 100001 + 3 && R.ranges[3] == two31 - 1);
        const RangePlan X = plan({0, 1}, {0, 3}, {100, 3 + two31}, 8);
        CHECK(X.error_code == FRISK_E_ARG && X.error == "range outside the scaffold (or empty, or of 2^31 bases or more) in row 1");
        CHECK(X.ranges.empty() && X.short_rows.empty() && X.long_rows.empty());
    }
    {   // the refusals, each with the first bad row
        const std::string idx = "sequence index out of range in row ", rng_ = "range outside the scaffold (or empty, or of 2^31 bases or more) in row ";
        CHECK(plan({0, 2}, {0, 0}, {10, 10}, 8).error == idx + "1");
        CHECK(plan({0, 0, -1}, {0, 0, 0}, {10, 10, 10}, 8).error == idx + "2");
        CHECK(plan({0, 0}, {0, 10}, {10, 10}, 8).error == rng_ + "1");                 // empty
        CHECK(plan({0}, {10}, {9}, 8).error == rng_ + "0");
        CHECK(plan({0}, {-1}, {9}, 8).error == rng_ + "0");
        CHECK(plan({0, 0, 0, 0}, {0, 0, 0, 5}, {10, 10, 100000, 100001}, 8).error == rng_ + "3");     // past the scaffold's end
        CHECK(plan({0, 1, 0}, {0, 0, 0}, {10, 100001, 100001}, 8).error == rng_ + "2");               // (the other scaffold's length does not count)
        CHECK(plan({0, 2}, {0, 0}, {10, 10}, 8).error_code == FRISK_E_ARG && plan({0}, {10}, {9}, 9, true, 5).error_code == FRISK_E_ARG);
    }
    return plans;
}

// frisk_refine_ranges' plan (range_plan.h: plan_refine).  Of an accepted plan: the rows of its RangePlan are the cores [a + Fe, b - Fe),
// Fe = min(flank, (b - a) / 4), and pass every check of plan_ranges; a row's geometry names its scaffold, a, b, Fe and the two
// clipped flanks, so that both search intervals lie inside the scaffold and new_start <= a + Fe < b - Fe <= new_stop can hold.
static long long check_refine_plan() {
    long long plans = 0;
    std::mt19937_64 rng(20241021);
    int64_t clipped_left = 0, clipped_right = 0, tiny = 0, capped = 0;
    for (int round = 0; round < 3000; ++round) {
        const int n_seq = 1 + int(rng() % 5);
        std::vector<int64_t> seq_len(static_cast<size_t>(n_seq)), seq_off(static_cast<size_t>(n_seq));
        int64_t off = 0;
        for (int s = 0; s < n_seq; ++s) {
            seq_len[size_t(s)] = 1 + int64_t(rng() % 300000);
            seq_off[size_t(s)] = off;
            off += seq_len[size_t(s)] + 1;
        }
        const int64_t n = int64_t(rng() % 40);
        std::vector<int32_t> si(static_cast<size_t>(n));
        std::vector<int64_t> a(static_cast<size_t>(n)), b(static_cast<size_t>(n));
        for (int64_t r = 0; r < n; ++r) {
            const int32_t s = int32_t(rng() % uint64_t(n_seq));
            const int64_t size = seq_len[size_t(s)];
            int64_t len = 1 + int64_t(rng() % uint64_t(size));
            if (rng() % 4 == 0) len = std::min<int64_t>(size, 1 + int64_t(rng() % 9));
            si[size_t(r)] = s;
            a[size_t(r)] = rng() % 5 == 0 ? 0 : (rng() % 5 == 0 ? size - len : int64_t(rng() % uint64_t(size - len + 1)));
            b[size_t(r)] = a[size_t(r)] + len;
        }
        const int kmin = 1 + int(rng() % 4), kmax = kmin + int(rng() % (13 - kmin)), num_cu = 1 + int(rng() % 300);
        const int32_t order = int32_t(kmin - 1 + int(rng() % (kmax - kmin + 1)));
        const int32_t flank = (rng() & 1) ? 1 + int32_t(rng() % 65536) : 1 + int32_t(rng() % 600);
        const bool all_long = kmax > 8 || rng() % 4 == 0;
        const RefinePlan R = plan_refine(n_seq, seq_len.data(), seq_off.data(), si.data(), a.data(), b.data(), n, flank, order, kmin, kmax, all_long, num_cu, 2);
        ++plans;
        CHECK(R.plan.error_code == FRISK_OK && int64_t(R.geom.size()) == n * FRISK_REFINE_GEOM);
        if (R.plan.error_code != FRISK_OK || int64_t(R.geom.size()) != n * FRISK_REFINE_GEOM) continue;
        std::vector<int64_t> ca(static_cast<size_t>(n)), cb(static_cast<size_t>(n));
        for (int64_t r = 0; r < n; ++r) {
            const int64_t* g = R.geom.data() + size_t(r) * FRISK_REFINE_GEOM;
            const int64_t L = seq_len[size_t(si[size_t(r)])], A = a[size_t(r)], B = b[size_t(r)], fe = g[3];
            CHECK(g[0] == seq_off[size_t(si[size_t(r)])] && g[1] == A && g[2] == B);
            CHECK(fe == std::min<int64_t>(flank, (B - A) / 4) && 0 <= fe && fe <= FRISK_REFINE_MAX_FLANK);
            CHECK(g[4] == std::min(fe, A) && g[5] == std::min(fe, L - B));
            CHECK(A - g[4] >= 0 && B + g[5] <= L && A + fe < B - fe + (fe == 0 ? 1 : 0) && A + fe < B - fe + 1);
            CHECK((fe == 0) == (B - A < 4));
            ca[size_t(r)] = A + fe; cb[size_t(r)] = B - fe;
            CHECK(ca[size_t(r)] < cb[size_t(r)]);
            clipped_left += g[4] < fe; clipped_right += g[5] < fe; tiny += fe == 0; capped += fe == flank;
        }
        check_one_plan(R.plan, seq_off, si, ca, cb, kmax, all_long, num_cu, 2, 0);
    }
    CHECK(clipped_left > 300 && clipped_right > 300 && tiny > 300 && capped > 300);      // (the sweep reaches them)
    // named cases on one batch
    const std::vector<int64_t> seq_len = {100000, 11}, seq_off = {0, 100001};
    auto plan = [&](const std::vector<int32_t>& si, const std::vector<int64_t>& a, const std::vector<int64_t>& b, int32_t flank, int32_t order,
                    int kmin = 1, int kmax = 8) {
        ++plans;
        return plan_refine(2, seq_len.data(), seq_off.data(), si.data(), a.data(), b.data(), int64_t(si.size()), flank, order, kmin, kmax, kmax > 8, 256, 2);
    };
    {   // n = 0; lengths 3, 4, 7, 8; a region at the first base, one at the last; 4F - 1, 4F, 4F + 1
        CHECK(plan({}, {}, {}, 500, 2).plan.error_code == FRISK_OK && plan({}, {}, {}, 500, 2).geom.empty());
        const RefinePlan R = plan({0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, {10, 10, 10, 10, 0, 99000, 5000, 5000, 5000, 0}, {13, 14, 17, 18, 3000, 100000, 6999, 7000, 7001, 11}, 500, 2);
        CHECK(R.plan.error_code == FRISK_OK);
        auto g = [&](int r, int k) { return R.geom[size_t(r * FRISK_REFINE_GEOM + k)]; };
        CHECK(g(0, 3) == 0 && g(1, 3) == 1 && g(2, 3) == 1 && g(3, 3) == 2);
        CHECK(R.plan.ranges[0] == 10 && R.plan.ranges[1] == 3 && R.plan.ranges[2] == 11 && R.plan.ranges[3] == 2 && R.plan.ranges[7] == 4);
        CHECK(g(4, 3) == 500 && g(4, 4) == 0 && g(4, 5) == 500 && g(5, 3) == 250 && g(5, 4) == 250 && g(5, 5) == 0);
        CHECK(g(6, 3) == 499 && g(7, 3) == 500 && g(8, 3) == 500 && R.plan.ranges[2 * 8 + 1] == 1001 && R.plan.ranges[2 * 6 + 1] == 1001);
        CHECK(g(9, 0) == 100001 && g(9, 3) == 2 && g(9, 4) == 0 && g(9, 5) == 0 && R.plan.ranges[18] == 100003 && R.plan.ranges[19] == 7);
    }
    {   // a core on either side of the short form's limit: 65 535 + 2 * 500 bases and one more
        const RefinePlan R = plan({0, 0}, {0, 0}, {66535, 66536}, 500, 2);
        CHECK(R.plan.short_rows == std::vector<int64_t>{0} && R.plan.long_rows == std::vector<int64_t>{1});
    }
    {   // the refusals: flank, order, then the rows as plan_ranges refuses them
        const char* chain = "the chain of order r reads the counts of order r + 1, which must lie in kmin .. kmax";
        for (int32_t f : {0, -1, 65537}) CHECK(plan({0}, {0}, {100}, f, 2).plan.error == "flank outside 1 .. 65536");
        CHECK(plan({0}, {0}, {100}, 65536, 2).plan.error_code == FRISK_OK && plan({0}, {0}, {100}, 1, 7).plan.error_code == FRISK_OK);
        CHECK(plan({0}, {0}, {100}, 500, 8).plan.error == chain && plan({0}, {0}, {100}, 500, -1).plan.error == chain);
        CHECK(plan({0}, {0}, {100}, 500, 1, 3, 5).plan.error == chain && plan({0}, {0}, {100}, 500, 5, 3, 5).plan.error == chain);
        CHECK(plan({0}, {0}, {100}, 500, 2, 3, 5).plan.error_code == FRISK_OK && plan({0}, {0}, {100}, 500, 11, 2, 12).plan.error_code == FRISK_OK);
        CHECK(plan({0, 2}, {0, 0}, {10, 10}, 500, 2).plan.error == "sequence index out of range in row 1");
        const std::string rng_ = "range outside the scaffold (or empty, or of 2^31 bases or more) in row ";
        CHECK(plan({0, 0}, {0, 10}, {10, 10}, 500, 2).plan.error == rng_ + "1" && plan({0}, {-1}, {9}, 500, 2).plan.error == rng_ + "0");
        CHECK(plan({1}, {0}, {12}, 500, 2).plan.error == rng_ + "0" && plan({1}, {0}, {12}, 500, 2).geom.empty());
        CHECK(plan({0}, {0}, {100}, 0, 99).plan.error_code == FRISK_E_ARG);
    }
    return plans;
}

// refine_math.h.  flog2 from below within 1 + 2^-20 units of 2^-32 bit of the long double logarithm (64-bit mantissa: 2^-20 of slack
// for its own rounding at 63 * 2^32), exact at the powers of two.  The change-point search as a workgroup runs it - nt threads' runs
// (refine_run), joined over each wave by the butterfly of refine_kernels.h and over the waves in order (refine_join), against the
// empty prefix (refine_pick) - against one plain scan that keeps the first maximum, over sequences full of ties.
static long long check_refine_math() {
    long long cuts = 0;
    std::mt19937_64 rng(77);
    auto check_log = [&](uint64_t x) {
        const long double d = std::log2(static_cast<long double>(x)) * 4294967296.0L - static_cast<long double>(refine_flog2(x));
        CHECK(d >= -1.0L / 1048576.0L && d < 1.0L + 1.0L / 1048576.0L);
    };
    for (uint64_t x = 1; x < 3000; ++x) check_log(x);
    for (int k = 1; k < 63; ++k) {
        CHECK(refine_flog2(uint64_t(1) << k) == int64_t(k) << 32);
        check_log((uint64_t(1) << k) - 1); check_log((uint64_t(1) << k) + 1);
    }
    for (int i = 0; i < 3000; ++i) check_log(1 + (rng() >> 2) % ((uint64_t(1) << 62) - 1));
    CHECK(refine_lp(0, 0) == -(int64_t(2) << 32) && refine_lp(3, 4) == (int64_t(2) << 32) - (int64_t(3) << 32));
    for (int round = 0; round < 4000; ++round) {
        const int nt = (round & 1) ? 1024 : 512;
        const int32_t n = round % 7 == 0 ? int32_t(rng() % 4) : (round % 5 == 0 ? int32_t(nt - 2 + rng() % 5) : int32_t(rng() % 5000));
        const int32_t Fe = int32_t(rng() % uint64_t(n + 2));
        const int span = 1 + int(rng() % 3);                    // small values: plateaus and ties everywhere
        std::vector<int64_t> x(static_cast<size_t>(n));
        for (auto& v : x) v = (rng() % 3 == 0) ? 0 : int64_t(rng() % uint64_t(2 * span + 1)) - span;
        if (round % 11 == 0) for (auto& v : x) v *= int64_t(1) << 38;
        std::vector<RefineCut> lane(static_cast<size_t>(nt));
        for (int t = 0; t < nt; ++t) lane[size_t(t)] = refine_run(n, t, nt, Fe, [&](int32_t i) { return x[size_t(i)]; });
        RefineCut total = {0, 0, 0, -1};
        for (int w = 0; w < nt / 64; ++w) {
            RefineCut* v = lane.data() + size_t(w) * 64;
            for (int d = 1; d < 64; d <<= 1) {
                RefineCut y[64];
                for (int l = 0; l < 64; ++l) y[l] = v[l ^ d];
                for (int l = 0; l < 64; ++l) v[l] = (l & d) ? refine_join(y[l], v[l]) : refine_join(v[l], y[l]);
            }
            for (int l = 1; l < 64; ++l) CHECK(v[l].sum == v[0].sum && v[l].best == v[0].best && v[l].arg == v[0].arg && v[l].ref == v[0].ref);
            total = w == 0 ? v[0] : refine_join(total, v[0]);
        }
        int64_t best, want_best = 0, run = 0, want_ref = 0;
        int32_t arg, want_arg = 0;
        refine_pick(total, best, arg);
        for (int32_t i = 0; i < n; ++i) {
            run += x[size_t(i)];
            if (i < Fe) want_ref += x[size_t(i)];
            if (run > want_best) { want_best = run; want_arg = i + 1; }
        }
        CHECK(best == want_best && arg == want_arg && total.ref == want_ref && total.sum == run);
        ++cuts;
    }
    return cuts;
}

// Phase A's plan (profile_plan.h).  plan_profile_launch over a sweep: the form follows the rule; the chunks of the forms with a table
// in LDS cover the range's words with no empty workgroup, on no more than one workgroup per CU; the big form's grid-stride loop
// (no chunks) has no idle workgroup either; the dynamic LDS fits a CU; grid = 0 exactly for an empty range.  Two named shapes against
// values worked out by hand.  plan_profile_pieces: ascending, disjoint, together [0, padded_len), each launch within what has arrived.
static long long check_profile_plan() {           // -> plans made
    long long plans = 0;
    const int64_t two30 = int64_t(1) << 30;
    const int64_t ranges[][2] = {
        {0, 0}, {77, 77},                                       // empty
        {0, 1}, {95, 96},                                       // one position
        {33, 60}, {64, 96},                                     // both ends inside one word / exactly one word
        {5, 100}, {31, 65}, {1000, 70001},                      // unaligned ends
        {0, 65535}, {0, 65536}, {0, 131072}, {17, 17 + 65535}, {17, 17 + 65536}, {17, 17 + 131072},
        {0, two30 - 1}, {0, two30}, {3, 3 + two30 - 1}, {3, 3 + two30},
        {0, 3300000000}, {31, 3300000000 - 7}};
    int64_t forms[3] = {0, 0, 0};
    for (int kmax = 1; kmax <= 12; ++kmax) for (int num_cu : {1, 2, 8, 256}) for (int one_pass = 0; one_pass < 2; ++one_pass) for (const auto& r : ranges) {
        const int64_t p0 = r[0], p1 = r[1], span = p1 - p0;
        const ProfileLaunch L = plan_profile_launch(kmax, num_cu, p0, p1, one_pass != 0);
        ++plans;
        const ProfileForm want = kmax > 8 ? PROFILE_FORM_BIG : (kmax == 8 && (one_pass || span >= two30)) ? PROFILE_FORM_ONE_PASS : PROFILE_FORM_LDS;
        CHECK(L.form == want);
        ++forms[L.form];
        int64_t words = 0;                                      // the words that hold a position of the range, counted one by one at both ends
        if (span > 0) words = (p1 - 1) / 32 - p0 / 32 + 1;
        CHECK(L.nwords == words);
        CHECK((L.grid == 0) == (span == 0) && L.grid >= 0);
        CHECK(L.halves == (want == PROFILE_FORM_LDS && kmax == 8 ? 2 : 1) && L.grid % L.halves == 0);
        CHECK(L.lds_bytes <= size_t(160) * 1024);
        if (want == PROFILE_FORM_BIG) {
            CHECK(L.threads == 256 && L.lds_bytes == 0 && L.chunk_words == 0 && L.grid <= 8 * num_cu);
            if (words > 0) CHECK(int64_t(L.grid - 1) * L.threads < words);                 // no workgroup without a word
            if (L.grid < 8 * num_cu) CHECK(int64_t(L.grid) * L.threads >= words);          // below the cap: one step of the loop
            continue;
        }
        CHECK(L.threads == 1024);
        CHECK(L.lds_bytes == (want == PROFILE_FORM_ONE_PASS ? size_t(131072) : std::max<size_t>(16, (size_t(1) << (2 * kmax)) * 4 / size_t(L.halves))));
        const int64_t chunks = L.grid / L.halves;
        if (words > 0) CHECK((chunks - 1) * L.chunk_words < words && words <= chunks * L.chunk_words);
        CHECK(chunks <= std::max<int64_t>(1, num_cu / L.halves));
        if (span > 0) CHECK(chunks <= std::max<int64_t>(1, span / 65536));
    }
    CHECK(forms[PROFILE_FORM_BIG] >= 100 && forms[PROFILE_FORM_ONE_PASS] >= 100 && forms[PROFILE_FORM_LDS] >= 100);    // (the sweep reaches each)
    {   // the bench shard (synth.c5_shard_lens(8, 0): 40 scaffolds, 410 630 532 bases, with their PADs 410 630 592 positions) at 256 CUs:
        // 12 832 206 words; 6 265 chunks of 65 536 positions would fit, 256 / 2 halves = 128 are allowed; ceil(12 832 206 / 128) = 100 252
        // words each (127 x 100 252 = 12 732 004 < 12 832 206 <= 128 x 100 252), so 128 chunks x 2 halves; 4^8 / 2 counters of 4 bytes
        const ProfileLaunch L = plan_profile_launch(8, 256, 0, 410630592, false);
        CHECK(L.form == PROFILE_FORM_LDS && L.grid == 256 && L.threads == 1024 && L.lds_bytes == 131072 && L.halves == 2);
        CHECK(L.chunk_words == 100252 && L.nwords == 12832206);
    }
    {   // the whole genome of that bench (all eight shards: 424 scaffolds, 3 285 019 936 positions >= 2^30: one pass) at 256 CUs:
        // 102 656 873 words, 50 125 chunks would fit, 256 are allowed; ceil(102 656 873 / 256) = 401 004 words each
        // (255 x 401 004 = 102 256 020 < 102 656 873 <= 256 x 401 004); 4^8 fields of 2 bytes
        const ProfileLaunch L = plan_profile_launch(8, 256, 0, 3285019936, false);
        CHECK(L.form == PROFILE_FORM_ONE_PASS && L.grid == 256 && L.threads == 1024 && L.lds_bytes == 131072 && L.halves == 1);
        CHECK(L.chunk_words == 401004 && L.nwords == 102656873);
    }
    {   // the corners: one CU at K = 8 (1 / 2 halves = 0 chunks allowed: one results, also of a single word), K = 1 (16 bytes), one position
        const ProfileLaunch A = plan_profile_launch(8, 1, 0, 1 << 20, false);
        CHECK(A.grid == 2 && A.halves == 2 && A.chunk_words == 32768);
        const ProfileLaunch A1 = plan_profile_launch(8, 1, 0, 32, false);
        CHECK(A1.grid == 2 && A1.halves == 2 && A1.chunk_words == 1);
        const ProfileLaunch B = plan_profile_launch(1, 256, 40, 41, false);
        CHECK(B.grid == 1 && B.lds_bytes == 16 && B.chunk_words == 1 && B.nwords == 1);
    }
    // the pieces of a streamed batch
    auto check_pieces = [&](const std::vector<int64_t>& piece_end, int64_t padded_len) {
        const std::vector<ProfilePiece> P = plan_profile_pieces(piece_end, padded_len);
        ++plans;
        CHECK(!P.empty() && P.size() <= piece_end.size());
        if (P.empty()) return P;
        int64_t at = 0, firsts = 0, lasts = 0;
        size_t prev_piece = 0;
        for (size_t k = 0; k < P.size(); ++k) {
            const ProfilePiece& L = P[k];
            CHECK(L.p0 == at && L.p1 >= L.p0);                  // ascending, disjoint, no gap
            at = L.p1;
            CHECK(L.piece < piece_end.size() && (k == 0 || L.piece > prev_piece));
            prev_piece = L.piece;
            if (L.piece < piece_end.size() && k + 1 < P.size()) CHECK(L.p1 <= (piece_end[L.piece] - 1) * 32);
            if (k > 0 && k + 1 < P.size()) CHECK(L.p1 > L.p0);  // between the first and the last only what adds positions
            firsts += L.first; lasts += L.last;
            CHECK(L.first == (k == 0) && L.last == (k + 1 == P.size()));
        }
        CHECK(at == padded_len && firsts == 1 && lasts == 1);
        CHECK(P.front().piece == 0 && P.back().piece + 1 == piece_end.size());
        return P;
    };
    for (int64_t piece_words : {1, 2, 3, 1000}) for (int64_t total_words : {1, 2, 3, 4, 7, 1000, 1001, 2999, 3000, 3001}) {
        std::vector<int64_t> piece_end;
        for (int64_t a = 0; a < total_words; a += piece_words) piece_end.push_back(std::min(total_words, a + piece_words));
        const std::vector<ProfilePiece> P = check_pieces(piece_end, total_words * 32);
        // pieces of one word: the first adds nothing (its only word waits for the next piece's) and launches all the same
        if (piece_words == 1 && total_words > 1 && !P.empty()) CHECK(P[0].p0 == 0 && P[0].p1 == 0 && P.size() == piece_end.size());
    }
    {
        const std::vector<ProfilePiece> one = check_pieces({5}, 160);                      // a single piece: first and last at once
        CHECK(one.size() == 1 && one[0].p0 == 0 && one[0].p1 == 160 && one[0].first && one[0].last);
        const std::vector<ProfilePiece> tail = check_pieces({4, 8, 9}, 288);               // a last piece of one word
        CHECK(tail.size() == 3 && tail[1].p1 == 224 && tail[2].p0 == 224 && tail[2].p1 == 288);
        const std::vector<ProfilePiece> none = check_pieces({4, 4, 8}, 256);               // a piece that adds nothing is left out
        CHECK(none.size() == 2 && none[0].p1 == 96 && none[1].piece == 2 && none[1].p0 == 96 && none[1].p1 == 256);
        const std::vector<ProfilePiece> ends = check_pieces({1, 1}, 32);                   // ... unless it is the first or the last
        CHECK(ends.size() == 2 && ends[0].p1 == 0 && ends[1].p0 == 0 && ends[1].p1 == 32);
    }
    return plans;
}

int main() {
    const long long profile_plans = check_profile_plan();
    const long long range_plans = check_range_plan();
    const long long refine_plans = check_refine_plan();
    const long long refine_cuts = check_refine_math();
    const long long plans = check_scan_schedule();
    const long long tile_shapes = check_scan_tiles();
    std::mt19937_64 rng(12345);
    const char alphabet[] = "ACGTacgtNnRYKM-*xACGTACGTACGT";
    for (int round = 0; round < 300; ++round) {
        const int n_seq = int(rng() % 6);
        std::vector<std::string> seqs;
        std::vector<int64_t> lens;
        for (int s = 0; s < n_seq; ++s) {
            const int64_t n = (round % 10 == 0 && s == 0) ? int64_t(1) << 22 : int64_t(rng() % 3000);      // (one batch in ten takes the threaded path)
            std::string q(size_t(n), 'A');
            for (auto& ch : q) ch = alphabet[rng() % (sizeof(alphabet) - 1)];
            for (int k = 0; k < 4 && n > 64; ++k) {                     // long runs: run merging across words and thread cuts
                const size_t a = rng() % size_t(n - 40), ln = rng() % 40 + (k == 0 ? 3000 % size_t(n - a) : 0);
                for (size_t i = a; i < std::min(size_t(n), a + ln); ++i) q[i] = (k & 1) ? 'N' : 'c';
            }
            seqs.push_back(q); lens.push_back(n);
        }
        std::vector<const uint8_t*> ptr;
        for (auto& q : seqs) ptr.push_back(reinterpret_cast<const uint8_t*>(q.data()));
        const int64_t P = frisk_pack2::padded_len(lens.data(), n_seq);
        std::vector<uint32_t> codes(size_t(P / 16), 0xDEADBEEFu);
        frisk_pack2::Runs R;
        frisk_pack2::pack_batch(ptr.data(), lens.data(), n_seq, codes.data(), R, 1 + int(rng() % 7), (round & 1) != 0);      // (odd rounds: the AVX-512 path where the host has it)
        // letter by letter
        std::vector<uint32_t> want(size_t(P / 16), 0u), inv(size_t(P / 32), 0u), low(size_t(P / 32), 0u);
        int64_t pos = 0;
        for (int s = 0; s < n_seq; ++s) {
            for (int64_t i = 0; i < lens[size_t(s)]; ++i, ++pos) {
                const uint8_t v = frisk_pack2::lut().t[uint8_t(seqs[size_t(s)][size_t(i)])];
                want[size_t(pos >> 4)] |= uint32_t(v & 3u) << (30 - 2 * int(pos & 15));
                if (v & 4u) inv[size_t(pos >> 5)] |= 0x80000000u >> (pos & 31);
                if (v & 8u) low[size_t(pos >> 5)] |= 0x80000000u >> (pos & 31);
            }
            ++pos;
        }
        CHECK(codes == want);
        for (int m = 0; m < 2; ++m) {
            const std::vector<int64_t>& runs = m ? R.low : R.inv;
            std::vector<uint32_t> got(size_t(P / 32), 0u);
            int64_t prev_end = -1;
            for (size_t k = 0; k + 1 < runs.size(); k += 2) {
                CHECK(runs[k] > prev_end && runs[k] < runs[k + 1] && runs[k + 1] <= P);
                prev_end = runs[k + 1];
                for (int64_t p = runs[k]; p < runs[k + 1]; ++p) got[size_t(p >> 5)] |= 0x80000000u >> (p & 31);
            }
            CHECK(got == (m ? low : inv));
            std::vector<int64_t> back;
            frisk_pack2::bitmap_runs((m ? low : inv).data(), lens.data(), n_seq, back);
            CHECK(back == runs);
        }
    }
    // HMM: series of awkward lengths (fewer windows than pieces, one window, constants)
    for (int64_t n : {int64_t(1), int64_t(2), int64_t(3), int64_t(255), int64_t(256), int64_t(257), int64_t(1000), int64_t(70001)}) {
        std::vector<double> x(static_cast<size_t>(n));
        std::normal_distribution<double> g0(-2.0, 0.3), g1(-0.5, 0.6);
        for (int64_t i = 0; i < n; ++i) x[size_t(i)] = ((i / 37) & 1) ? g1(rng) : g0(rng);
        if (n == 3) x[0] = x[1] = x[2] = 0.25;
        const frisk_hmm::Fit f = frisk_hmm::fit(x.data(), n, 10, 1e-2, 1e-3, 1e-2);
        CHECK(f.m.covars[0] > 0 && f.m.covars[1] > 0);
        std::vector<int64_t> off{0, n / 3, n / 3, n};               // (an empty segment in the middle)
        std::vector<int8_t> path(static_cast<size_t>(n), int8_t(9));
        frisk_hmm::viterbi_segments(x.data(), off.data(), 3, f.m, path.data());
        for (int8_t s : path) CHECK(s == 0 || s == 1);
    }
    // FASTA reader + seek index: files of every awkward form the Python mirror accepts; where an index can be built, every record read
    // back through it must equal the parser's bytes
    {
        const std::string path = "/tmp/frisk_san_host.fa";
        const std::vector<std::string> files = {
            "", ">only_header", ">a\nACGT\n>b\n\n>c\nAC\nGT", ">a desc\r\nACGT\r\nAC\r\n>b\r\nTT\r\n", "ACGT\n>late\nAAA\n", ">x\nACGTACGT\nACGTACGT\nAC\n>y\nAAAA\nAAAA\nAAAA",
            ">r\nACGT\nACG\nACGT\n", ">b\nAC GT\n\nAC\n", ">t\n" + std::string(200000, 'G') + "\n>u\n" + std::string(77, 'a'), "\n\n>z\nNNNN\n\n", ">\nAC\n>",
            ">w\nACGTAC\nACGTAC\nACGTAC\n\n>v\nAC\n"};
        std::vector<std::string> all(files);
        for (int big = 0; big < 2; ++big) {             // > 16 MB: the readers' multi-threaded path, runs across lines, blocks and chunk cuts
            std::string t;
            const char letters[] = "ACGTACGTACGTacgtN";
            while (t.size() < (size_t(20) << 20)) {
                t += ">rec" + std::to_string(t.size()) + " x\n";
                size_t n = (rng() % 7 == 0) ? rng() % 50 : rng() % 3000000;
                const size_t width = big ? 61 : 60;
                std::string q(n, 'A');
                for (auto& ch : q) ch = letters[rng() % (sizeof(letters) - 1)];
                for (int k = 0; k < 6 && n > 5000; ++k) {
                    const size_t a = rng() % (n - 4000), ln = rng() % 4000;
                    for (size_t i = a; i < a + ln; ++i) q[i] = (k & 1) ? 'N' : char(q[i] | 0x20);
                }
                for (size_t i = 0; i < n; i += width) { t.append(q, i, std::min(width, n - i)); t += big ? "\r\n" : "\n"; }
            }
            all.push_back(t);
        }
        for (const std::string& text : all) {
            { std::ofstream fh(path, std::ios::binary); fh << text; }
            frisk_fasta::Records rec;
            std::string err;
            const bool ok = frisk_fasta::parse(path.c_str(), rec, err, 1 + int(rng() % 5));
            if (!ok) continue;
            int64_t total = 0;
            for (int64_t n : rec.lens) total += n + 1;
            CHECK(int64_t(rec.stage.size()) >= total && rec.names.size() == rec.lens.size());
            {   // the fused reader (no staging buffer) against parse() + pack_stage(), both letter widths
                for (int wide = 0; wide < 2; ++wide) {
                    frisk_fasta::Records r2;
                    frisk_fasta::CodeVec c2;
                    frisk_pack2::Runs R2;
                    bool fused = false;
                    CHECK(frisk_fasta::parse_pack(path.c_str(), r2, c2, R2, err, 1 + int(rng() % 5), &fused, wide != 0));
                    CHECK(r2.names == rec.names && r2.lens == rec.lens);
                    const int64_t P = frisk_pack2::padded_len(rec.lens.data(), int32_t(rec.lens.size()));
                    std::vector<uint32_t> c1(size_t(P / 16));
                    frisk_pack2::Runs R1;
                    frisk_pack2::pack_stage(rec.stage.data(), rec.lens.data(), int32_t(rec.lens.size()), c1.data(), R1, 3, false);
                    CHECK(c2.size() == c1.size() && std::equal(c1.begin(), c1.end(), c2.begin()));
                    CHECK(R1.inv == R2.inv && R1.low == R2.low);
                }
            }
            frisk_fasta::MappedFile f(path.c_str());
            std::vector<frisk_fasta::FaiEntry> idx;
            std::string why;
            if (!frisk_fasta::build_index(f, idx, why)) continue;
            CHECK(idx.size() == rec.lens.size());
            int64_t off = 0;
            for (size_t r = 0; r < idx.size() && r < rec.lens.size(); ++r) {
                CHECK(idx[r].len == rec.lens[r]);
                std::vector<uint8_t> got(size_t(idx[r].len) + 1, 0);
                frisk_fasta::read_range_mt(f, idx[r], 0, idx[r].len, got.data(), 3);
                CHECK(std::memcmp(got.data(), rec.stage.data() + off, size_t(idx[r].len)) == 0);
                if (idx[r].len > 5) {
                    frisk_fasta::read_range(f, idx[r], 3, idx[r].len - 5, got.data());
                    CHECK(std::memcmp(got.data(), rec.stage.data() + off + 3, size_t(idx[r].len - 5)) == 0);
                }
                off += rec.lens[r] + 1;
            }
            const std::string ip = path + ".fai";
            CHECK(frisk_fasta::write_index(ip.c_str(), f, idx, why));
            std::vector<frisk_fasta::FaiEntry> back;
            const bool rd = frisk_fasta::read_index(ip.c_str(), f, back, why);
            if (!(rd && back.size() == idx.size())) std::printf("read_index: %s (file of %zu bytes, %zu records)\n", why.c_str(), text.size(), idx.size());
            CHECK(rd && back.size() == idx.size());
            ::unlink(ip.c_str());
        }
        ::unlink(path.c_str());
    }
    std::printf("%s (%d failed checks; %lld scan schedules; %lld tile plans; %lld range plans; %lld refine plans; %lld refine cuts; %lld profile plans; AVX-512 packer %s)\n", fails ? "FAILED" : "ok", fails, plans, tile_shapes, range_plans, refine_plans, refine_cuts, profile_plans, frisk_pack2::have_avx512() ? "exercised" : "not available on this host");
    return fails ? 1 : 0;
}
