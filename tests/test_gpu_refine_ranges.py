"""frisk_refine_ranges (csrc/refine_kernels.h) on the device: every output column equal to the numpy restatement of
frisk_amd/refine.py - integers, compared with == - on the range set of tests/ranges_cases.py through both forms, at the named edges
(batch ends, clipped flanks, the N run, the soft-masked run, the shortest lengths, 4F +- 1, a dropped core, the periodic-N scaffold,
the 11-base scaffold, either side of the short form's limit, the orphan hand-over), on a tie plateau under both tie rules and on the
planted island; what the header promises about reproducibility and about rejected calls."""
import functools
import os

import numpy as np
import pytest

import ranges_cases as R
from golden_util import INPUTS

pytestmark = pytest.mark.gpu

GRID = [(1, 8, 0), (1, 8, 2), (1, 8, 7), (3, 5, 2), (3, 5, 4), (2, 9, 1)]
FLANKS = [1, 31, 500, 4096]
COLS = ["status", "nn", "new_start", "new_stop", "gain_start", "gain_stop", "flank_used"]
COARSE = [(29000, 43000), (30500, 41500), (29500, 41000), (31000, 43500), (30000, 42000)]


@functools.lru_cache(maxsize=None)
def want(kmin, kmax, r, F, rows, seqs=None):
    """The restatement's columns, computed once per case and shared (rows, seqs: tuples)."""
    from frisk_amd import refine
    sym, _ = R.profile(kmin, kmax)
    return refine.refine_rows(list(seqs) if seqs is not None else R.scaffolds(), sym, kmin, list(rows), F, r, kmax=kmax)


def same(tag, got, exp, ia=None):
    for c in COLS:
        g, w = getattr(got, c), getattr(exp, c)
        w = w if ia is None else w[ia]
        bad = np.nonzero(g.astype(np.int64) != w.astype(np.int64))[0]
        assert bad.size == 0, "%s: column %s differs in %d rows, first %d: device %d, restatement %d" % (
            tag, c, bad.size, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))
    return True


# ------------------------------------------------------------------------------------------------ the range set, both forms
@pytest.mark.parametrize("big", [False, True], ids=["auto", "big"])
@pytest.mark.parametrize("kmin,kmax,r", GRID)
def test_range_set_equals_the_restatement(kmin, kmax, r, big):
    rows = tuple(R.range_set(kmax))
    moved = 0
    with R.engine(kmin, kmax) as e:
        for F in FLANKS:
            got = e.refine_ranges(*R.arrays(rows), F, r, big=big)
            assert e.kernel_ms(8) > 0.0
            exp = want(kmin, kmax, r, F, rows)
            same("refine k=%d..%d r=%d F=%d %s" % (kmin, kmax, r, F, "big" if big else "auto"), got, exp)
            s, a, b = R.arrays(rows)
            assert (got.new_start <= a + got.flank_used).all() and (b - got.flank_used <= got.new_stop).all()
            assert (got.gain_start >= 0).all() and (got.gain_stop >= 0).all()
            moved += int(((got.new_start != a) | (got.new_stop != b)).sum())
            assert int((exp.status == 0).sum()) >= 2
    assert moved >= 100


# -------------------------------------------------------------------------------------------------------------- named edges
def _orphans(seq, a, b):
    """Entries of the K = 8 short form's orphan list for the slice [a, b): positions whose longest valid word has 7 letters."""
    ok = np.frombuffer(seq[a:b].upper(), dtype=np.uint8)
    ok = np.isin(ok, np.frombuffer(b"ACGT", dtype=np.uint8))
    n = ok.size
    runs = np.zeros(n + 1, dtype=np.int64)
    for j in range(n - 1, -1, -1):
        runs[j] = runs[j + 1] + 1 if ok[j] else 0
    return int((np.minimum(runs[:n], 8) == 7).sum())


def edge_rows(F):
    seqs = R.scaffolds()
    n0, n1, n2 = len(seqs[0]), len(seqs[1]), len(seqs[2])
    rows = [(0, 0, 2100), (0, 0, 77), (3, 4, 11), (3, 0, 11), (3, 0, 8), (3, 1, 9),           # the batch's first and last base; 11 bases
            (0, 10, 2400), (0, n0 - 2400, n0 - 20), (1, 100, 9000), (1, n1 - 9000, n1 - 100),  # a flank clipped on one side only
            (0, 1400, 1500), (0, 1540, 1640), (0, 1450, 1590), (0, 1300, 1520), (0, 1520, 1900), (0, 1100, 1540), (0, 1500, 2000),
            (0, 1000, 1500),                                                                    # inside, beside, across the N run
            (0, 2000, 2560), (0, 2700, 3400), (0, 2400, 3000), (0, 2200, 3300),                 # the soft-masked run [2540, 2840)
            (0, 64, 67), (0, 64, 68), (0, 64, 71), (0, 64, 72), (0, 500, 503), (0, 500, 504),   # lengths 3, 4, 7, 8
            (1, 5000, 5000 + 4 * F - 1), (1, 5000, 5000 + 4 * F), (1, 5000, 5000 + 4 * F + 1),  # 4F - 1, 4F, 4F + 1
            (0, 1490, 1550), (0, 1480, 1560), (0, 2500, 2880),                                  # cores the N rule drops
            (2, 0, 650), (2, 5, 3000), (2, 0, n2), (2, 30000, 40000),                           # an N every ten bases
            (1, 0, 65535 + 2 * F), (1, 0, 65536 + 2 * F), (1, 1000, 1000 + 65535 + 2 * F)]      # a core at the short form's limit
    return tuple(r for r in rows if r[2] <= len(seqs[r[0]]))


@pytest.mark.parametrize("big", [False, True], ids=["auto", "big"])
@pytest.mark.parametrize("kmin,kmax,r,F", [(1, 8, 2, 500), (1, 8, 7, 31), (1, 8, 0, 2000), (3, 5, 4, 500), (2, 9, 1, 4096), (2, 9, 8, 500),
                                           (1, 8, 4, 65536)])
def test_named_edges_equal_the_restatement(kmin, kmax, r, F, big):
    rows = edge_rows(F)
    exp = want(kmin, kmax, r, F, rows)
    with R.engine(kmin, kmax) as e:
        got = e.refine_ranges(*R.arrays(rows), F, r, big=big)
    same("edges k=%d..%d r=%d F=%d" % (kmin, kmax, r, F), got, exp)
    s, a, b = R.arrays(rows)
    assert int((exp.status == 0).sum()) >= 3                            # dropped cores: new = old, no gain, the flank as computed
    drop = exp.status == 0
    assert (got.new_start[drop] == a[drop]).all() and (got.new_stop[drop] == b[drop]).all() and (got.flank_used[drop] > 0).all()
    short = (b - a) < 4
    assert int(short.sum()) >= 2 and (got.flank_used[short] == 0).all() and (got.new_start[short] == a[short]).all()
    if F <= 500:
        assert {int(v) for v in got.flank_used[[rows.index((1, 5000, 5000 + 4 * F + d)) for d in (-1, 0, 1)]]} == {F - 1, F}
    if r + 1 == 9:                                                      # scaffold 2's blocks of nine bases hold one valid word each
        on2 = s == 2
        assert int(on2.sum()) >= 3 and (got.gain_start[on2] + got.gain_stop[on2] > 0).any()


def test_orphan_hand_over_gives_the_same_integers():
    """Scaffold 2 has an N every ten bases: each block of nine leaves one orphan 7-mer.  With F = 10 the cores of (2, 0, 660) and
    (2, 0, 670) are [10, 650) and [10, 660): 64 orphans fill the short form's list, 65 overflow it and the row reaches the long form
    through the device list, in the same call."""
    seqs = R.scaffolds()
    rows = ((2, 0, 660), (2, 0, 670), (2, 0, 65535), (2, 20, 670), (0, 100, 700))
    assert _orphans(seqs[2], 10, 650) == 64 and _orphans(seqs[2], 10, 660) == 65
    for r in (2, 6, 7):
        exp = want(1, 8, r, 10, rows)
        assert (exp.flank_used == 10).all() and (exp.status == R.KEPT).all()
        with R.engine(1, 8) as e:
            auto = e.refine_ranges(*R.arrays(rows), 10, r)
            big = e.refine_ranges(*R.arrays(rows), 10, r, big=True)
        same("orphan hand-over r=%d" % r, auto, exp)
        same("orphan hand-over r=%d, long form" % r, big, exp)


# --------------------------------------------------------------------------------------------------------------------- ties
def test_tie_plateaus_go_to_the_shorter_region():
    """host | N run | island | N run | host, the host ending and starting AT-rich at the runs, the island GC-rich: q is 0 over an N run
    and over the r bases behind it, whose words hold an N, so both cumulative sums are flat there - at their maximum, since the base
    in front of a plateau loses and the one behind it gains.  The restatement's profiles show the ties (26 + r cuts each); the start
    goes to the plateau's last cut, the stop to its first: the N runs stay outside, on the device as in the restatement."""
    from frisk_amd import refine
    rng = np.random.default_rng(11)
    seq = (R._bases(rng, 2994, 0.3) + b"ATATAA" + b"N" * 25 + b"GCGGCC" + R._bases(rng, 3988, 0.7) + b"GCCGGC" + b"N" * 25 + b"AATATT" +
           R._bases(rng, 2994, 0.3))
    seqs = (seq,)
    rows = ((0, 2900, 7200), (0, 3100, 7000), (0, 2990, 7060))
    sym, _ = R.profile(1, 8)
    for r, F in ((2, 300), (0, 300), (1, 300), (3, 300)):
        exp = want(1, 8, r, F, rows, seqs)
        for i, row in enumerate(rows):
            (t, Gs), (u, Ge) = refine.cut_profiles(list(seqs), sym, 1, row, F, r, kmax=8)
            ts, us = t[Gs == Gs.max()], u[Ge == Ge.max()]
            assert ts.size == 26 + r and us.size == 26 + r, (r, row, ts.size, us.size)              # the restatement shows a tie
            assert int(exp.new_start[i]) == int(ts.max()) == 3025 + r and int(exp.new_stop[i]) == int(us.min()) == 7025
        with R.engine(1, 8, seqs=list(seqs)) as e:
            for big in (False, True):
                same("ties r=%d %s" % (r, "big" if big else "auto"), e.refine_ranges(*R.arrays(rows), F, r, big=big), exp)


# ---------------------------------------------------------------------------------------------------------- planted island
def test_planted_island_is_found_to_the_base():
    """The GC 0.7 island at [30000, 42000) of scaffold 1, from five coarse regions up to 1 500 bases off, F = 2000: the restatement
    gives 30006 and 41999 at r = 0, 1, 2 (tests/test_refine_cpu.py); the device the same, and within 50 bases of the truth."""
    rows = tuple((1, a, b) for a, b in COARSE)
    with R.engine(1, 8) as e:
        for r in (0, 1, 2):
            got = e.refine_ranges(*R.arrays(rows), 2000, r)
            same("island r=%d" % r, got, want(1, 8, r, 2000, rows))
            print("order %d: starts %s stops %s" % (r, got.new_start.tolist(), got.new_stop.tolist()))
            assert (np.abs(got.new_start - 30000) <= 50).all() and (np.abs(got.new_stop - 42000) <= 50).all()


# ---------------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("kmin,kmax,r", [(1, 8, 2), (1, 8, 7), (1, 6, 2), (2, 9, 1)])
def test_rows_do_not_depend_on_the_call(kmin, kmax, r):
    import torch
    rows = tuple(R.range_set(kmax))
    s, a, b = R.arrays(rows)
    n, F = len(rows), 500
    score_cols = ["status", "nn", "kld", "gc", "pi", "si", "cri"]
    with R.engine(kmin, kmax) as e:
        scan0 = e.scan(5000, 1000, rip=True)
        score0 = e.score_ranges(s, a, b, rip=True)
        first = e.refine_ranges(s, a, b, F, r)
        again = e.refine_ranges(s, a, b, F, r)
        perm = np.random.default_rng(5).permutation(n)
        shuffled = e.refine_ranges(s[perm], a[perm], b[perm], F, r)
        cut = n // 3
        halves = [e.refine_ranges(s[:cut], a[:cut], b[:cut], F, r), e.refine_ranges(s[cut:], a[cut:], b[cut:], F, r)]
        copies = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
        one = rows.index((1, 29000, 43000))
        many = e.refine_ranges(np.full(copies, s[one]), np.full(copies, a[one]), np.full(copies, b[one]), F, r)
        scan1 = e.scan(5000, 1000, rip=True)
        score1 = e.score_ranges(s, a, b, rip=True)
    exp = want(kmin, kmax, r, F, rows)
    same("first", first, exp)
    same("again", again, exp)
    same("permuted", shuffled, exp, ia=perm)
    same("first part", halves[0], exp, ia=np.arange(cut))
    same("second part", halves[1], exp, ia=np.arange(cut, n))
    same("copies", many, exp, ia=np.full(copies, one))
    assert (first.new_start[one], first.new_stop[one]) != (29000, 43000)
    assert len(scan0) > 0
    R.same_columns(scan0, scan1, ["seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri"])
    R.same_columns(score0, score1, score_cols)


# --------------------------------------------------------------------------------------------------------------- rejections
def test_rejected_calls_launch_nothing_and_write_nothing():
    import ctypes
    from frisk_amd import _ffi
    from frisk_amd.engine import Engine
    known = ((1, 29000, 43000), (0, 64, 64 + 513))
    n0 = len(R.scaffolds()[0])

    def code(e, rows, F=500, r=2, **kw):
        with pytest.raises(_ffi.FriskHipError) as err:
            e.refine_ranges(*R.arrays(rows), F, r, **kw)
        return err.value.code

    def refines(e, tag):
        same(tag, e.refine_ranges(*R.arrays(known), 500, 2), want(1, 8, 2, 500, known))

    with Engine(1, 8) as e:
        assert code(e, known) == _ffi.E_ARG                                     # no resident batch
        e.load(R.scaffolds())
        assert code(e, known) == _ffi.E_STATE                                   # no finalised profile
        sym, meta = R.profile(1, 8)
        e.profile_set(sym, *[int(v) for v in meta])
        for bad in ([(4, 0, 10)], [(-1, 0, 10)], [(0, -1, 10)], [(0, 10, 10)], [(0, 10, 9)], [(0, 0, n0 + 1)], [(3, 0, 12)],
                    list(known) + [(0, 5, n0 + 1)]):
            assert code(e, bad) == _ffi.E_ARG, bad
        refines(e, "after rejected rows")
        for F in (0, -1, 65537):
            assert code(e, known, F=F) == _ffi.E_ARG, F
        for r in (-1, 8, 12):
            assert code(e, known, r=r) == _ffi.E_ARG, r
        refines(e, "after a rejected flank and order")
        e.load_fasta_shard(os.path.join(INPUTS, "markov_islands.fa"), 400, 150, 0, 1)       # a tiled batch
        assert code(e, [(0, 0, 10)]) == _ffi.E_ARG
        e.load(R.scaffolds())
        # a null array, one at a time; a bad flank with arrays in place; n = 0: nothing is written in any of them
        s, a, b = R.arrays(known[:1])
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
        lib = _ffi.lib()
        st = np.full(1, 77, np.uint32)
        out = [np.full(1, -7, np.int64) for _ in range(6)]
        full = [p(st)] + [p(x) for x in out]
        for hole in range(7):
            args = list(full)
            args[hole] = None
            assert lib.frisk_refine_ranges(e._ctx, p(s), p(a), p(b), 1, 0, 500, 2, *args) == _ffi.E_ARG, hole
        for hole in range(3):
            rows3 = [p(s), p(a), p(b)]
            rows3[hole] = None
            assert lib.frisk_refine_ranges(e._ctx, *rows3, 1, 0, 500, 2, *full) == _ffi.E_ARG, hole
        assert lib.frisk_refine_ranges(e._ctx, p(s), p(a), p(b), 1, 0, 0, 2, *full) == _ffi.E_ARG
        assert lib.frisk_refine_ranges(e._ctx, p(s), p(a), p(b), 1, 0, 500, 8, *full) == _ffi.E_ARG
        assert lib.frisk_refine_ranges(e._ctx, p(s), p(a), p(b), -1, 0, 500, 2, *full) == _ffi.E_ARG
        assert lib.frisk_refine_ranges(e._ctx, None, None, None, 0, 0, 500, 2, *([None] * 7)) == _ffi.OK
        assert lib.frisk_refine_ranges(e._ctx, p(s), p(a), p(b), 0, 0, 500, 2, *full) == _ffi.OK
        assert st[0] == 77 and all(x[0] == -7 for x in out)
        refines(e, "after null arrays")
        e.profile_reset()
        assert code(e, known) == _ffi.E_STATE
        e.profile_add(); e.profile_finalize()
        assert len(e.refine_ranges(*R.arrays(known), 500, 2)) == 2
    with Engine(3, 5) as e:                                                     # the order's rule follows kmin
        e.load(R.scaffolds())
        sym, meta = R.profile(3, 5)
        e.profile_set(sym, *[int(v) for v in meta])
        assert code(e, known, r=1) == _ffi.E_ARG and code(e, known, r=5) == _ffi.E_ARG
        same("k=3..5", e.refine_ranges(*R.arrays(known), 500, 2), want(3, 5, 2, 500, known))
