"""frisk_score_ranges (csrc/range_kernels.h) on the device: every row of the range set of tests/ranges_cases.py against the
reference's scan-loop iteration on the slice - status, nn, GC and the RIP indices exactly, the KLD within
kld_oracle_hp.bound(scale) (C_KLD = 32) of the extended-precision value - on both forms, at the hand-over between them, against
frisk_scan on the window grid, and for what the header promises about reproducibility and rejected calls.  Each case prints its
worst normalised KLD error."""
import os

import numpy as np
import pytest

import kld_oracle_hp as H
import ranges_cases as R
from golden_util import INPUTS, same_float
from oracle import frisk_oracle_np as N

pytestmark = pytest.mark.gpu


def _same_rows(a, b, rip):
    return R.same_columns(a, b, R.score_columns(rip))


def _take(res, idx, rip):
    from frisk_amd.engine import ScanResult
    cols = ["seq_index", "start", "stop", "status", "nn", "kld", "gc"] + (["pi", "si", "cri"] if rip else [])
    return ScanResult(**{c: getattr(res, c)[idx] for c in cols})


# ------------------------------------------------------------------------------------------------ the range set, both forms
# (that the set holds its classes - dropped by the N rule, no max-mer, ZeroDivisionError - is asserted in tests/test_regions_cpu.py)
@pytest.mark.parametrize("big", [False, True], ids=["auto", "big"])
@pytest.mark.parametrize("kmin,kmax", R.ORDERS)
def test_range_set_against_the_oracles(kmin, kmax, big):
    rows, exp = R.expected(kmin, kmax)
    rip = kmin <= 2 <= kmax
    with R.engine(kmin, kmax) as e:
        res = e.score_ranges(*R.arrays(rows), rip=rip, big=big)
        ms = e.kernel_ms(4)
    assert ms > 0.0
    assert not (res.status & R.JUMPBACK).any()
    R.check("ranges k=%d..%d %s" % (kmin, kmax, "big" if big else "auto"), res, exp)


def test_one_range_at_k10():
    rows = [(1, 28000, 44000)]
    prof = H.profile(R.scaffolds(), 1, 10)
    ig = N.genome_ivom_table(prof[0], prof[1], 1, 10)
    exp = R.expect_rows(R.scaffolds(), prof, ig, rows, 1, 10)
    assert exp[0]["flag"] == H.OK
    with R.engine(1, 10, prof=prof) as e:
        R.check("ranges k=1..10", e.score_ranges(*R.arrays(rows), rip=True), exp)
        R.check("ranges k=1..10 big", e.score_ranges(*R.arrays(rows), rip=True, big=True), exp)


# --------------------------------------------------------------------------------------------------------- orphan hand-over
def test_orphan_list_hands_over_to_the_long_form():
    """s2 = 7000 x (9 random + N): one orphan 7-mer per 10 bases at K = 8.  640 bases hold exactly the 64 the LDS list takes, 650
    one more - that range reaches the long form through the device list -, (0, 65535) holds 6553."""
    rows = [(2, 0, 640), (2, 0, 650), (2, 0, 65535), (2, 10, 650), (0, 100, 700)]
    prof = R.profile(1, 8)
    exp = R.expect_rows(R.scaffolds(), prof, R._ig(1, 8), rows, 1, 8)
    assert all(x["flag"] == H.OK for x in exp)
    with R.engine(1, 8) as e:
        auto = e.score_ranges(*R.arrays(rows), rip=True)
        big = e.score_ranges(*R.arrays(rows), rip=True, big=True)
    R.check("orphan hand-over", auto, exp)
    assert _same_rows(auto, big, True)


# ----------------------------------------------------------------------------------------------------------- grid agreement
@pytest.mark.parametrize("fasta", ["markov_islands.fa", "nheavy.fa"])
def test_ranges_agree_with_the_scan_on_its_own_grid(fasta):
    """Every candidate window of frisk_scan (w = 400, i = 150) passed as a range - a jumpback window by its slice."""
    from frisk_amd.engine import Engine
    w, inc, kmin, kmax = 400, 150, 1, 8
    seqs = H.read_fasta(os.path.join(INPUTS, fasta))
    prof = H.profile(seqs, kmin, kmax)
    with Engine(kmin, kmax) as e:
        e.load_fasta(os.path.join(INPUTS, fasta))
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        scan = e.scan(w, inc, rip=True)
        jump = (scan.status & R.JUMPBACK) != 0
        start = np.where(jump, scan.start, scan.start - 1)
        res = e.score_ranges(scan.seq_index, start, scan.stop, rip=True)
    assert len(scan) > 0 and np.array_equal(scan.status & ~np.uint32(R.JUMPBACK), res.status)
    for c in ("gc", "pi", "si", "cri"):
        assert getattr(scan, c).tobytes() == getattr(res, c).tobytes(), c
    hp = H.scan_hp(seqs, prof, kmin, kmax, w, inc)
    assert np.array_equal(hp["cand"], np.nonzero(res.kept)[0])
    checked = 0
    for k, flag, scale in zip(hp["cand"].tolist(), hp["flag"].tolist(), hp["scale"].tolist()):
        a, b = float(scan.kld[k]), float(res.kld[k])
        if flag == H.OK:
            assert abs(a - b) <= 2 * float(H.bound(scale)), (k, a, b)
            checked += 1
        else:
            assert same_float(a, b), (k, a, b)
    assert checked >= min(10, len(scan) // 2)
    assert np.isnan(res.kld[~res.kept]).all() and np.isnan(res.gc[~res.kept]).all()


# ---------------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("kmin,kmax", [(1, 8), (1, 6), (2, 9)])
def test_rows_do_not_depend_on_the_call(kmin, kmax):
    import torch
    rows, _ = R.expected(kmin, kmax)
    rip = True
    s, a, b = R.arrays(rows)
    n = len(rows)
    with R.engine(kmin, kmax) as e:
        before = e.scan(5000, 1000, rip=True)
        first = e.score_ranges(s, a, b, rip=rip)
        again = e.score_ranges(s, a, b, rip=rip)
        perm = np.random.default_rng(5).permutation(n)
        shuffled = e.score_ranges(s[perm], a[perm], b[perm], rip=rip)
        cut = n // 3
        halves = [e.score_ranges(s[:cut], a[:cut], b[:cut], rip=rip), e.score_ranges(s[cut:], a[cut:], b[cut:], rip=rip)]
        copies = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
        one = rows.index((0, 64, 64 + R.T_SHORT + 1))
        many = e.score_ranges(np.full(copies, s[one]), np.full(copies, a[one]), np.full(copies, b[one]), rip=rip)
        after = e.scan(5000, 1000, rip=True)
    assert _same_rows(first, again, rip)
    assert _same_rows(_take(first, perm, rip), shuffled, rip)
    assert _same_rows(_take(first, np.arange(cut), rip), halves[0], rip) and _same_rows(_take(first, np.arange(cut, n), rip), halves[1], rip)
    assert _same_rows(_take(first, np.full(copies, one), rip), many, rip)
    assert len(before) > 0
    for c in ("seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri"):
        assert getattr(before, c).tobytes() == getattr(after, c).tobytes(), c


# --------------------------------------------------------------------------------------------------------------- rejections
def test_rejected_calls_launch_nothing_and_leave_the_state():
    from frisk_amd import _ffi
    from frisk_amd.engine import Engine
    known = [(0, 64, 64 + 513)]
    exp = R.expect_rows(R.scaffolds(), R.profile(1, 8), R._ig(1, 8), known, 1, 8)
    n0 = len(R.scaffolds()[0])

    def code(e, rows, **kw):
        with pytest.raises(_ffi.FriskHipError) as err:
            e.score_ranges(*R.arrays(rows), **kw)
        return err.value.code

    with Engine(1, 8) as e:
        assert code(e, known) == _ffi.E_ARG                                     # no resident batch
        e.load(R.scaffolds())
        assert code(e, known) == _ffi.E_STATE                                   # no finalised profile
        sym, meta = R.profile(1, 8)
        e.profile_set(sym, *[int(v) for v in meta])
        for bad in ([(4, 0, 10)], [(-1, 0, 10)], [(0, -1, 10)], [(0, 10, 10)], [(0, 10, 9)], [(0, 0, n0 + 1)], [(3, 0, 12)],
                    known + [(0, 5, n0 + 1)]):
            assert code(e, bad) == _ffi.E_ARG, bad
            R.check("after a rejected call", e.score_ranges(*R.arrays(known), rip=True), exp)
        # a tiled batch (one rank's window tiles: its offsets and lengths are the tiles', not the scaffolds'), under the same
        # finalised profile; a plain load afterwards scores the known range again
        e.load_fasta_shard(os.path.join(INPUTS, "markov_islands.fa"), 400, 150, 0, 1)
        assert code(e, [(0, 0, 10)]) == _ffi.E_ARG
        e.load(R.scaffolds())
        R.check("after a tiled batch", e.score_ranges(*R.arrays(known), rip=True), exp)
        # a null required array; n = 0 touches nothing
        s, a, b = R.arrays(known)
        out = np.zeros(1)
        st, nn = np.zeros(1, np.uint32), np.full(1, -7, np.int64)
        p = lambda x: x.ctypes.data_as(__import__("ctypes").c_void_p)           # noqa: E731
        lib = _ffi.lib()
        assert lib.frisk_score_ranges(e._ctx, p(s), p(a), p(b), 1, 0, p(st), None, p(out), None, None, None, p(nn)) == _ffi.E_ARG
        assert lib.frisk_score_ranges(e._ctx, p(s), p(a), p(b), 1, _ffi.SCAN_RIP, p(st), p(out), p(out), None, None, None, p(nn)) == _ffi.E_ARG
        assert lib.frisk_score_ranges(e._ctx, None, None, None, 0, 0, None, None, None, None, None, None, None) == _ffi.OK
        assert nn[0] == -7
        e.profile_reset()
        assert code(e, known) == _ffi.E_STATE
        e.profile_add(); e.profile_finalize()
        R.check("after a new profile", e.score_ranges(*R.arrays(known), rip=True), exp)
    with Engine(3, 5) as e:                                                     # RIP needs the dinucleotides
        e.load(R.scaffolds())
        sym, meta = R.profile(3, 5)
        e.profile_set(sym, *[int(v) for v in meta])
        assert code(e, known, rip=True) == _ffi.E_ARG
        assert len(e.score_ranges(*R.arrays(known))) == 1


def test_a_stop_of_2_31_is_refused():
    """Refused by the scaffold bound: the clause for ranges of 2^31 bases or more needs a 2 Gb scaffold and has no test."""
    from frisk_amd import _ffi
    with R.engine(1, 6) as e:
        with pytest.raises(_ffi.FriskHipError) as err:
            e.score_ranges([0], [0], [1 << 31])
        assert err.value.code == _ffi.E_ARG


# --------------------------------------------------------------------------------------------------------------- query mode
def test_query_ranges_against_the_host_profile():
    from frisk_amd.engine import Engine
    host = H.read_fasta(os.path.join(INPUTS, "host.fa"))
    query = H.read_fasta(os.path.join(INPUTS, "query.fa"))
    kmin, kmax = 1, 8
    prof = H.profile(host, kmin, kmax)
    ig = N.genome_ivom_table(prof[0], prof[1], kmin, kmax)
    rows = []
    for s, q in enumerate(query):
        n = len(q)
        rows += [(s, 0, n), (s, 0, min(n, 700)), (s, max(0, n - 333), n), (s, n // 3, n // 3 + min(64, n - n // 3))]
    exp = R.expect_rows(query, prof, ig, rows, kmin, kmax)
    assert sum(x["flag"] == H.OK for x in exp) >= 2
    with Engine(kmin, kmax) as e:
        e.load_fasta(os.path.join(INPUTS, "host.fa"))
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        e.load_fasta(os.path.join(INPUTS, "query.fa"))
        res = e.score_ranges(*R.arrays(rows), rip=True)
    R.check("query ranges against the host profile", res, exp)
