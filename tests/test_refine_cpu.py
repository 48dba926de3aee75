"""frisk_refine_ranges and python -m frisk_amd.regions --refine, as far as a machine without a GPU can tell: the symbol, the
fixed-point logarithm and the table of frisk_amd/refine.py against long-double logarithms, the restatement against an independent
brute force in Python integers (every candidate cut summed from scratch), the planted island of tests/ranges_cases.py, and the module
end to end on an engine whose refine_ranges is the restatement."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import ranges_cases as R
import test_regions_cpu as TR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LD = np.longdouble
TWO32 = LD(4294967296.0)
GRID = [(1, 8, 0), (1, 8, 2), (1, 8, 7), (3, 5, 2), (3, 5, 4), (2, 9, 1)]
FLANKS = [1, 31, 500, 4096]
COLS = ["status", "nn", "new_start", "new_stop", "gain_start", "gain_stop", "flank_used"]
COARSE = [(29000, 43000), (30500, 41500), (29500, 41000), (31000, 43500), (30000, 42000)]


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_refine_symbol_is_declared_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    from frisk_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "frisk_hip.h")).read(), flags=re.S)
    i64 = r"\s*int64_t\s*\*\s*"
    assert re.search(r"\bint\s+frisk_refine_ranges\s*\(\s*frisk_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*seq_index\s*,\s*const\s+int64_t\s*\*\s*"
                     r"start\s*,\s*const\s+int64_t\s*\*\s*stop\s*,\s*int64_t\s+n\s*,\s*uint32_t\s+flags\s*,\s*int32_t\s+flank\s*,\s*int32_t\s+order\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*," + i64 + "nn," + i64 + "new_start," + i64 + "new_stop," + i64 + "gain_start," + i64 +
                     "gain_stop," + i64 + r"flank_used\s*\)", text)
    table = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert table["frisk_refine_ranges"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_uint32, C.c_int32, C.c_int32] + [C.c_void_p] * 7)
    lib = _ffi.lib()
    assert lib.frisk_refine_ranges(None, None, None, None, 0, 0, 500, 2, None, None, None, None, None, None, None) == _ffi.E_ARG
    assert lib.frisk_last_kernel_ms(None, 8) == -1.0
    from frisk_amd import refine
    from frisk_amd.engine import Engine
    from frisk_amd.hotpath import HotPath
    assert callable(Engine.refine_ranges) and callable(HotPath.refineRegions) and refine.MAX_FLANK == _ffi.REFINE_MAX_FLANK == 65536


# ------------------------------------------------------------------------------------------------------------- arithmetic
def _sample():
    rng = np.random.default_rng(20241021)
    xs = list(range(1, 3000)) + [2 ** k + d for k in range(1, 63) for d in (-1, 1)] + [int(v) for v in rng.integers(1, 2 ** 62, 3000)]
    return np.array(sorted(set(xs)), dtype=np.uint64)


def _log2_units(x):
    """2^32 log2 x in long double (64-bit mantissa: the uint64 converts exactly; at 63 * 2^32 its rounding is below 2^-24 units)."""
    return np.log2(np.asarray(x, dtype=np.uint64).astype(LD)) * TWO32


def test_flog2_lies_within_one_unit_below_the_logarithm():
    from frisk_amd import refine
    x = _sample()
    assert x.size >= 6000 and np.finfo(LD).nmant >= 63
    d = _log2_units(x) - refine.flog2(x).astype(LD)
    print("flog2: %d values, 2^32 log2 x - flog2 x in [%.6f, %.6f]" % (x.size, float(d.min()), float(d.max())))
    slack = LD(2.0) ** -20
    assert (d >= -slack).all() and (d < 1 + slack).all()
    powers = np.array([1 << k for k in range(63)], dtype=np.uint64)
    assert np.array_equal(refine.flog2(powers), np.arange(63, dtype=np.int64) << 32)         # exact at the powers of two
    for bad in (0, 1 << 63):
        with pytest.raises(ValueError):
            refine.flog2(np.array([bad], dtype=np.uint64))


def test_qtab_lies_within_two_units_of_the_log_ratio():
    """Four logarithms, each up to 1 + 2^-20 below its value, two with either sign: 2 + 2^-19 units."""
    from frisk_amd import refine
    rng = np.random.default_rng(5)
    worst = 0.0
    for x, scale_i, scale_h in ((1, 50, 10 ** 6), (3, 3, 10 ** 4), (5, 40, 10 ** 9), (2, 10 ** 4, 10 ** 15), (4, 0, 0)):
        isl = rng.integers(0, scale_i + 1, 4 ** x)
        host = rng.integers(0, scale_h + 1, 4 ** x)
        isl[:4] = 0                                                                          # an unseen context: lp = log2(1 / 4)
        q = refine.qtab(isl, host)
        assert q.dtype == np.int64 and q.shape == (4 ** x,)
        ti, th = np.repeat(isl.reshape(-1, 4).sum(1), 4), np.repeat(host.reshape(-1, 4).sum(1), 4)
        want = (_log2_units(isl + 1) - _log2_units(ti + 4)) - (_log2_units(host + 1) - _log2_units(th + 4))
        err = np.abs(q.astype(LD) - want)
        worst = max(worst, float(err.max()))
        assert (err <= 2 + LD(2.0) ** -19).all()
    print("qtab: worst |error| %.4f units of 2^-32 bit" % worst)
    assert np.array_equal(refine.lp_table([0, 0, 0, 0]), np.full(4, -2 << 32))               # log2(1 / 4), exactly


# ------------------------------------------------------------------------------------------------------------ brute force
@functools.lru_cache(maxsize=None)
def _flog2_int(x):
    e = x.bit_length() - 1
    m, f = x << (63 - e), 0
    for _ in range(32):
        p = m * m
        hi = p >> 64
        f <<= 1
        if hi >= 1 << 63:
            f |= 1
            m = hi
        else:
            m = (hi << 1) | ((p & ((1 << 64) - 1)) >> 63)
    return (e << 32) + f


def _code(word):
    c = 0
    for ch in word:
        c = 4 * c + "ATGC".index(ch)
    return c


def brute_row(seqs, sym, kmin, kmax, row, F, r):
    """One row by the definition, in Python integers and strings: nothing shared with refine.py."""
    s, a, b = row
    seq = seqs[s].decode("ascii")
    L, x = len(seq), r + 1
    Fe = min(F, (b - a) // 4)
    core = seq[a + Fe:b - Fe]
    nn = sum(ch not in "ACGT" for ch in core)
    out = dict(status=0, nn=nn, new_start=a, new_stop=b, gain_start=0, gain_stop=0, flank_used=Fe)
    if nn >= 0.3 * len(core):
        return out
    up = seq.upper()
    S = len(core) - nn
    ok = [ch in "ACGT" for ch in up[a + Fe:b - Fe]]
    run, ntop = 0, 0
    for v in ok:
        run = run + 1 if v else 0
        ntop += run >= kmax
    out["status"] = R.KEPT | (R.NO_MAXMER if ntop == 0 else 0) | (R.ZERO_WEIGHT if ntop > 0 and kmin - 1 <= S <= kmax - 1 else 0)
    if Fe == 0:
        return out
    island = {}
    for i in range(a + Fe, b - Fe - x + 1):
        w = up[i:i + x]
        if all(ch in "ACGT" for ch in w):
            island[w] = island.get(w, 0) + 1
    off = sum(4 ** i for i in range(kmin, x))

    def q_of(w):
        ti = sum(island.get(w[:-1] + ch, 0) for ch in "ATGC")
        c = _code(w)
        th = sum(int(sym[off + (c & ~3) + d]) for d in range(4))
        return (_flog2_int(island.get(w, 0) + 1) - _flog2_int(ti + 4)) - (_flog2_int(int(sym[off + c]) + 1) - _flog2_int(th + 4))

    memo = {}

    def q(j):
        if j - r < 0:
            return 0
        w = up[j - r:j + 1]
        if not all(ch in "ACGT" for ch in w):
            return 0
        if w not in memo:
            memo[w] = q_of(w)
        return memo[w]

    lo_s, hi_s = max(0, a - Fe), a + Fe
    qs = [q(j) for j in range(lo_s, hi_s)]
    G = {t: sum(qs[t - lo_s:]) for t in range(lo_s, hi_s + 1)}                  # every cut from scratch
    top = max(G.values())
    out["new_start"] = max(t for t, g in G.items() if g == top)
    out["gain_start"] = top - G[a]
    lo_e, hi_e = b - Fe, min(L, b + Fe)
    qe = [q(j) for j in range(lo_e, hi_e)]
    G = {u: sum(qe[:u - lo_e]) for u in range(lo_e, hi_e + 1)}
    top = max(G.values())
    out["new_stop"] = min(u for u, g in G.items() if g == top)
    out["gain_stop"] = top - G[b]
    return out


def cpu_rows():
    """Rows on the four scaffolds: both ends of the batch, a flank clipped on one side, the N run, the soft-masked run, the shortest
    lengths, 4F +- 1 for the small flanks, a dropped core, the scaffold with an N every ten bases, the 11-base scaffold, the island."""
    seqs = R.scaffolds()
    n0, n1, n2 = len(seqs[0]), len(seqs[1]), len(seqs[2])
    rows = [(0, 0, 77), (0, 0, 2100), (0, n0 - 100, n0), (0, 10, 400), (0, n0 - 410, n0 - 20),
            (0, 1400, 1500), (0, 1540, 1640), (0, 1450, 1590), (0, 1505, 1535), (0, 1300, 1520), (0, 1520, 1900), (0, 1100, 1540),
            (0, 2400, 3000), (0, 2540, 2840), (0, 2000, 2560), (0, 0, n0),
            (0, 64, 67), (0, 64, 68), (0, 64, 71), (0, 64, 72), (0, 500, 503), (0, 500, 504), (0, 500, 505),
            (0, 200, 323), (0, 200, 324), (0, 200, 325), (0, 100, 2099), (0, 100, 2100), (0, 100, 2101),
            (1, 29000, 43000), (1, 0, n1), (1, 69000, n1), (1, 100, 5000),
            (2, 0, 650), (2, 5, 3000), (2, 0, n2),
            (3, 0, 8), (3, 0, 11), (3, 1, 9), (3, 0, 3), (3, 4, 11)]
    return rows


@pytest.mark.parametrize("kmin,kmax,r", GRID)
def test_restatement_equals_the_brute_force(kmin, kmax, r):
    from frisk_amd import refine
    seqs = R.scaffolds()
    sym, _ = R.profile(kmin, kmax)
    rows = cpu_rows()
    moved = dropped = short = 0
    for F in FLANKS:
        got = refine.refine_rows(seqs, sym, kmin, rows, F, r, kmax=kmax)
        for i, row in enumerate(rows):
            want = brute_row(seqs, sym, kmin, kmax, row, F, r)
            for c in COLS:
                assert int(getattr(got, c)[i]) == want[c], (F, row, c, int(getattr(got, c)[i]), want[c])
            assert want["gain_start"] >= 0 and want["gain_stop"] >= 0
            Fe = want["flank_used"]
            assert want["new_start"] <= row[1] + Fe and row[2] - Fe <= want["new_stop"]
            moved += (want["new_start"], want["new_stop"]) != row[1:]
            dropped += want["status"] == 0
            short += Fe == 0
    assert moved >= 40 and dropped >= 4 and short >= 8
    for bad_f, bad_r in ((0, r), (65537, r), (500, kmax), (500, kmin - 2), (500, -1)):
        with pytest.raises(ValueError):
            refine.refine_rows(seqs, sym, kmin, rows[:1], bad_f, bad_r, kmax=kmax)


def test_planted_island_is_found_to_the_base():
    """Scaffold 1: 70 000 bases at GC 0.3 with a GC 0.7 island at [30000, 42000); five coarse regions up to 1 500 bases off, F = 2000.
    The restatement's values (profile of the four scaffolds, kmin..kmax = 1..8): every coarse region and each of r = 0, 1, 2 gives
    new_start = 30006 and new_stop = 41999 - 6 and 1 bases off, within the 50 asserted.  (The bases at [30000, 30006) and at 41999
    were drawn from the island's distribution but happen to favour the host's.)"""
    from frisk_amd import refine
    seqs = R.scaffolds()
    sym, _ = R.profile(1, 8)
    rows = [(1, a, b) for a, b in COARSE]
    for r in (0, 1, 2):
        got = refine.refine_rows(seqs, sym, 1, rows, 2000, r, kmax=8)
        print("order %d: starts %s stops %s" % (r, got.new_start.tolist(), got.new_stop.tolist()))
        assert (np.abs(got.new_start - 30000) <= 50).all() and (np.abs(got.new_stop - 42000) <= 50).all()
        assert (got.status == R.KEPT).all() and (got.flank_used == 2000).all()
    # a flank that does not reach the boundary: the cut goes to the flank's edge (30500: island all the way; 43000: host all the
    # way, give or take the first bases' own ratios)
    got = refine.refine_rows(seqs, sym, 1, [(1, 31000, 43500)], 500, 2, kmax=8)
    assert 30500 <= int(got.new_start[0]) <= 30550 and 43000 <= int(got.new_stop[0]) <= 43050


# ------------------------------------------------------------------------------------------ the module on a restating engine
class _RefineEngine(TR._Engine):
    """TR._Engine whose refine_ranges is the numpy restatement."""
    calls = []

    def load(self, seqs):
        self.raw_seqs = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in seqs]
        super().load(seqs)

    def refine_ranges(self, seq_index, start, stop, flank, order, big=False):
        from frisk_amd import refine
        sym, _ = self.profile
        seq_index, start, stop = np.asarray(seq_index, np.int32), np.asarray(start, np.int64), np.asarray(stop, np.int64)
        res = refine.refine_rows(self.raw_seqs, sym, self.kmin, list(zip(seq_index.tolist(), start.tolist(), stop.tolist())), flank, order,
                                 kmax=self.kmax)
        res.seq_index, res.start, res.stop = seq_index, start, stop
        _RefineEngine.calls.append((int(flank), int(order)))
        return res


@pytest.fixture
def refine_regions(monkeypatch):
    from frisk_amd import hotpath, regions
    monkeypatch.setattr(hotpath, "Engine", _RefineEngine)
    real_init = hotpath.HotPath.__init__

    def init(self, kMin, kMax, device=0, cache_dir=None, use_cache=True):
        real_init(self, kMin, kMax, device=device, cache_dir=None, use_cache=use_cache)
    monkeypatch.setattr(hotpath.HotPath, "__init__", init)
    _RefineEngine.calls = []
    return regions


def test_module_end_to_end_table_bed_and_unchanged_scores(refine_regions, tmp_path):
    from frisk_amd import postprocess as pp, refine
    fa, bed, chr1 = TR._inputs(tmp_path)
    regs = [("tiny", 5, 9, "zw"), ("chr1", 0, 100, "geneA"), ("chr1", 115, 155, "gap"), ("chr1", 0, 3, "."), ("chr1", 199, 200, "lastbase"),
            ("chr1", 0, 1, "firstbase")]
    base = ["-H", fa, "-k", "4", "--bed", bed]
    assert refine_regions.main(base + ["-t", str(tmp_path / "plain")]) == 0
    assert refine_regions.main(base + ["-t", str(tmp_path / "ref"), "--refine", "20"]) == 0
    assert _RefineEngine.calls == [(20, 2)]                                             # min(max(2, kmin - 1), kmax - 1) at 1..4
    assert refine.default_order(1, 8) == 2 and refine.default_order(5, 8) == 4 and refine.default_order(1, 2) == 1
    plain = (tmp_path / "plain" / "region_scores.tsv").read_bytes()
    assert (tmp_path / "ref" / "region_scores.tsv").read_bytes() == plain
    assert not (tmp_path / "plain" / "region_refined.tsv").exists() and not (tmp_path / "plain" / "regions_refined.bed").exists()
    lines = (tmp_path / "ref" / "region_refined.tsv").read_text().split("\n")
    assert lines[0].split("\t") == refine_regions.REFINE_COLUMNS == ["name", "start", "stop", "length", "id", "newStart", "newStop", "newLength",
                                                                    "shiftStart", "shiftStop", "llrStart", "llrStop", "flank", "windowKLD",
                                                                    "newKLD", "note"]
    assert lines[-1] == "" and len(lines) == len(regs) + 2
    seqs = [chr1.encode(), b"ACGTTGCAacg"]
    from oracle import frisk_oracle_np as N
    sym = np.asarray(N.genome_profile([chr1, "ACGTTGCAacg"], 1, 4)[0], dtype=np.int64)
    index = {"chr1": 0, "tiny": 1}
    want = refine.refine_rows(seqs, sym, 1, [(index[n], a, b) for n, a, b, _ in regs], 20, 2, kmax=4)
    scores = [l.split("\t") for l in plain.decode().split("\n")[1:-1]]
    notes = []
    for i, ((name, a, b, ident), line) in enumerate(zip(regs, lines[1:-1])):
        f = line.split("\t")
        ns, ne = int(want.new_start[i]), int(want.new_stop[i])
        assert f[:5] == [name, str(a + 1), str(b), str(b - a), ident]
        assert f[5:10] == [str(ns + 1), str(ne), str(ne - ns), str(ns - a), str(ne - b)], f
        assert f[10:12] == [pp.py2_str(int(want.gain_start[i]) / 2.0 ** 32), pp.py2_str(int(want.gain_stop[i]) / 2.0 ** 32)]
        assert f[12] == str(int(want.flank_used[i])) and f[13] == scores[i][4]
        notes.append(f[15])
    assert notes == [".", ".", "unresolved", "short", "short", "short"]
    assert int(want.flank_used[0]) == 1 and int(want.flank_used[1]) == 20 and int(want.flank_used[2]) == 10
    assert (int(want.new_start[1]), int(want.new_stop[1])) != (0, 100)                  # (the scored region moves)
    # the BED holds the refined regions, and a plain run on it prints the newKLD column
    bed2 = (tmp_path / "ref" / "regions_refined.bed").read_text()
    assert bed2 == "".join("%s\t%d\t%d\t%s\n" % (n, int(want.new_start[i]), int(want.new_stop[i]), ident) for i, (n, _, _, ident) in enumerate(regs))
    assert refine_regions.main(["-H", fa, "-k", "4", "--bed", str(tmp_path / "ref" / "regions_refined.bed"), "-t", str(tmp_path / "again")]) == 0
    again = [l.split("\t") for l in (tmp_path / "again" / "region_scores.tsv").read_text().split("\n")[1:-1]]
    assert [l.split("\t")[14] for l in lines[1:-1]] == [f[4] for f in again]
    # other file names, an explicit order; no regions: the headers
    assert refine_regions.main(base + ["-t", str(tmp_path / "ref"), "--refine", "7", "--refineOrder", "0", "--refineOutfile", "r.tsv",
                                       "--refinedBed", "r.bed"]) == 0
    assert _RefineEngine.calls[-1] == (7, 0) and (tmp_path / "ref" / "r.tsv").is_file() and (tmp_path / "ref" / "r.bed").is_file()
    empty = tmp_path / "empty.bed"
    empty.write_text("# nothing\n")
    assert refine_regions.main(["-H", fa, "-k", "4", "--bed", str(empty), "-t", str(tmp_path / "e"), "--refine", "20"]) == 0
    assert (tmp_path / "e" / "region_refined.tsv").read_text() == "\t".join(refine_regions.REFINE_COLUMNS) + "\n"
    assert (tmp_path / "e" / "regions_refined.bed").read_text() == ""


def test_refused_combinations_end_the_run_before_any_device_work(tmp_path, caplog):
    from frisk_amd import regions
    bed = tmp_path / "r.bed"
    bed.write_text("chr1\t0\t100\n")
    out = tmp_path / "t"
    base = ["-H", str(tmp_path / "absent.fa"), "-t", str(out), "--bed", str(bed)]       # (the host FASTA does not even exist)
    for extra, word in ((["--refine", "500", "--donors", "d.fa"], "--donors"), (["--refine", "500", "--null", "markov"], "--null"),
                        (["--refine", "500", "--null", "host"], "--null"), (["--refine", "500", "--topKmers", "5"], "--topKmers"),
                        (["--refine", "0"], "1..65536"), (["--refine", "65537"], "1..65536"), (["--refine", "-3"], "1..65536"),
                        (["--refine", "500", "--refineOrder", "8"], "--refineOrder"), (["--refine", "500", "--refineOrder", "-1"], "--refineOrder"),
                        (["--refine", "500", "-m", "4", "-k", "6", "--refineOrder", "2"], "--refineOrder")):
        caplog.clear()
        assert regions.main(base + extra) == 1, extra
        assert word in caplog.text, (extra, caplog.text)
        assert not out.exists()
    assert regions.refine_problem(regions.build_parser().parse_args(base + ["--refine", "65536", "--refineOrder", "7"])) is None
    assert regions.refine_problem(regions.build_parser().parse_args(base + ["--refine", "1", "-m", "4", "-k", "6"])) is None     # order 3
