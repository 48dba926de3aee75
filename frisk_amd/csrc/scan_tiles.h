// scan_tiles.h - which candidate windows a scaffold has, and window-tile sharding: which rank scores which windows, keeps which
// bases resident and counts which positions in phase A.  Pure integer arithmetic.  No HIP here: frisk_scan_plan (frisk_abi.hip) and
// the two shard loaders (frisk_seq.hip) call it; tools/exp/san_host.cpp sweeps its invariants on a CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// what one rank holds of one scaffold (frisk_ctx::Batch::Tile)
struct Tile {
    int32_t scaf;               // index of the scaffold in the FASTA (what seq_index reports)
    int64_t size;               // length of the whole scaffold
    int64_t base0;              // position inside the scaffold of the tile's first base
    int64_t j0, ncand;          // first window index inside the scaffold and number of windows scored here
    int32_t kind;               // as ScafDesc::kind
    int64_t own0, own1;         // [own0, own1): scaffold positions whose k-mers THIS rank counts in phase A
};

// candidate windows of one scaffold (crawlGenome, L194-251)
inline void plan_scaffold(int64_t size, int32_t w, int32_t inc, bool all, int64_t& ncand, int32_t& kind) {
    const double limit = double(w) + ((double(w) * 0.75) - double(inc));      // L211 / L222, evaluated as CPython does
    if (double(size) <= limit) {
        kind = 1;
        ncand = all ? 1 : 0;
    } else {
        kind = 0;
        ncand = (size - inc + 1 > 0) ? (size - inc) / inc + 1 : 0;            // len(range(0, size-inc+1, inc)), L228
    }
}

// [lo, hi) of the rank-th of `world` near-equal contiguous parts of range(n)
inline void split_range(int64_t n, int rank, int world, int64_t& lo, int64_t& hi) {
    const int64_t base = n / world, extra = n % world;
    lo = rank * base + std::min<int64_t>(rank, extra);
    hi = lo + base + (rank < extra ? 1 : 0);
}

// Window-tile sharding: the job's candidate windows are numbered in output order over ALL scaffolds and cut
// into `world` contiguous ranges; a rank keeps, per scaffold, the bases of its windows - [j0*i, (j1-1)*i + w), reaching back
// to size-w where its range includes the scaffold's jumpback windows (L230-243) - and counts (phase A) the k-mers that start
// in [j0*i, j1*i), or up to the scaffold's end behind its last window, so that every base of the genome is counted by
// exactly one rank; K-1 bases beyond that range are kept for the words that start in it.  Scaffolds without windows go to
// the rank whose range holds their position in the numbering.
inline std::vector<Tile> plan_tiles(const std::vector<int64_t>& lens, int32_t w, int32_t inc, bool all, int /* kmax: tile_end()'s */, int rank,
                                    int world, int64_t& c0, int64_t& c1) {
    std::vector<int64_t> ncand(lens.size()), first(lens.size());
    std::vector<int32_t> kind(lens.size());
    int64_t total = 0;
    for (size_t s = 0; s < lens.size(); ++s) {
        plan_scaffold(lens[s], w, inc, all, ncand[s], kind[s]);
        first[s] = total;
        total += ncand[s];
    }
    split_range(total, rank, world, c0, c1);
    std::vector<Tile> tiles;
    for (size_t s = 0; s < lens.size(); ++s) {
        const int64_t size = lens[s];
        const int64_t ja = std::max<int64_t>(c0, first[s]) - first[s], jb = std::min<int64_t>(c1, first[s] + ncand[s]) - first[s];
        Tile t;
        t.scaf = int32_t(s); t.size = size; t.kind = kind[s];
        if (jb > ja) {
            t.j0 = ja; t.ncand = jb - ja;
            if (kind[s] == 1) { t.base0 = 0; t.own0 = 0; t.own1 = size; tiles.push_back(t); continue; }
            int64_t a = ja * inc;
            if ((jb - 1) * inc + w > size) a = std::min<int64_t>(a, std::max<int64_t>(0, size - w));    // jumpback windows
            t.base0 = a;
            t.own0 = ja * inc;
            t.own1 = (jb == ncand[s]) ? size : jb * inc;
            tiles.push_back(t);             // (what it keeps resident ends at tile_end())
        } else if (ncand[s] == 0) {
            // no windows at all: counted by the rank whose candidate range holds this scaffold's place in the numbering
            const bool mine = (first[s] >= c0 && first[s] < c1) || (first[s] == total && rank == world - 1) ||
                              (total == 0 && rank == world - 1);
            if (!mine) continue;
            t.j0 = 0; t.ncand = 0; t.base0 = 0; t.own0 = 0; t.own1 = size;
            tiles.push_back(t);
        }
    }
    return tiles;
}

// one past the last scaffold position a tile keeps resident
inline int64_t tile_end(const Tile& t, int32_t w, int32_t inc, int kmax) {
    if (t.ncand == 0 || t.kind == 1) return t.size;
    int64_t b = (t.j0 + t.ncand - 1) * inc + w;
    if (b > t.size) b = t.size;
    return std::max<int64_t>(b, std::min<int64_t>(t.size, t.own1 + kmax - 1));
}
