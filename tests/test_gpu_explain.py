"""frisk_explain_ranges (csrc/explain_kernels.h) on the device: the score columns against frisk_score_ranges byte for byte, every
listed k-mer against the extended-precision per-k-mer oracle of tests/explain_oracle.py (the term within C_TERM eps64 s_k, C_TERM =
16 from a CPU calibration), the order and completeness of the lists, ties, both forms and the hand-over between them, what the
header promises about reproducibility and rejected calls, and the --topKmers command line.  Each case of the range set prints its
worst normalised term error."""
import os

import numpy as np
import pytest

import explain_oracle as X
import kld_oracle_hp as H
import ranges_cases as R
from golden_util import INPUTS

pytestmark = pytest.mark.gpu

LD = H.LD
SCORE = ["status", "nn", "kld", "gc"]
TOP = ["n_present", "code", "count", "pw", "pg", "term"]
NONE = 0xFFFFFFFF


def _cols(rip):
    return SCORE + (["pi", "si", "cri"] if rip else []) + TOP          # thirteen with rip


_same = R.same_columns


def _empty(res, r, j0=0):
    return ((res.code[r, j0:] == NONE).all() and (res.count[r, j0:] == 0).all() and np.isnan(res.pw[r, j0:]).all()
            and np.isnan(res.pg[r, j0:]).all() and np.isnan(res.term[r, j0:]).all())


def _key(term):
    """The device's own bits as sortable numbers: -0.0 equals +0.0."""
    return np.where(term == 0.0, 0.0, term)


def check_explain(tag, res, exp, kmax, top_n):
    """Clauses (a)-(e) on every row; returns (worst normalised term error, rows checked, adjacent bit-equal pairs, rows under (e))."""
    worst, checked, ties, complete = 0.0, 0, 0, 0
    assert res.code.shape == (len(exp), top_n)
    for r, e in enumerate(exp):
        where = "%s row %d" % (tag, r)
        st = int(res.status[r])
        assert int(res.n_present[r]) == (0 if e is None else e["m"]), (where, int(res.n_present[r]))
        if st != R.KEPT:
            assert e is None or e["flag"] != H.OK, where
            assert _empty(res, r), where
            continue
        assert e is not None and e["flag"] == H.OK, where           # (the set holds no DEGENERATE row: tests/test_regions_cpu.py)
        m = e["m"]
        L = min(top_n, m)
        assert _empty(res, r, L), where
        code, term = res.code[r, :L].astype(np.int64), res.term[r, :L]
        # (a) distinct, present, exact counts
        at = np.searchsorted(e["present"], code)
        assert len(set(code.tolist())) == L and (at < m).all() and np.array_equal(e["present"][np.minimum(at, m - 1)], code), where
        assert np.array_equal(res.count[r, :L].astype(np.int64), e["count"][at]), where
        # (b) term, pw, pg within their bounds
        err = X.normalised_term_error(term, e["t_hp"][at], e["s"][at])
        worst = max(worst, float(err.max()))
        assert (err <= X.C_TERM).all(), "%s: a term %.2f eps64 s_k off (C_TERM = %g)" % (where, float(err.max()), X.C_TERM)
        for got, hp in ((res.pw[r, :L], e["pw"][at]), (res.pg[r, :L], e["pg"][at])):
            assert (np.abs(got.astype(LD) - hp) <= H.C_IVOM * (kmax + 2) * LD(H.EPS64) * hp).all(), where
        # (c) sorted by the device's own bits: term descending, equal terms by ascending code
        k = _key(term)
        assert ((k[:-1] > k[1:]) | ((k[:-1] == k[1:]) & (code[:-1] < code[1:]))).all(), where
        ties += int((term[:-1].view(np.uint64) == term[1:].view(np.uint64)).sum())
        # (d) nothing outside the list is provably larger than its last entry
        out = np.ones(m, bool)
        out[at] = False
        last = at[-1]
        b = X.term_bound(np.asarray(e["s"], dtype=np.float64))
        assert (e["t_hp"][out] <= e["t_hp"][last] + LD(b[last]) + b[out].astype(LD)).all(), where
        # (e) a complete list sums to the row's KLD
        if m <= top_n:
            assert L == m and not out.any(), where
            total = term.astype(LD).sum()
            assert abs(total - LD(float(res.kld[r]))) <= (X.C_TERM + H.C_KLD) * H.EPS64 * e["scale"], where
            complete += 1
        checked += 1
    print("%-44s rows %4d  complete lists %3d  worst normalised term error %6.2f" % (tag, checked, complete, worst))
    return worst, checked, ties, complete


# ------------------------------------------------------------------------------------------------ the range set, both forms
CASES = [(kmin, kmax, 64) for kmin, kmax in R.ORDERS + [(1, 3), (2, 2)]] + [(1, 8, 1), (1, 8, 5)]


@pytest.mark.parametrize("big", [False, True], ids=["auto", "big"])
@pytest.mark.parametrize("kmin,kmax,top_n", CASES)
def test_range_set_against_the_per_kmer_oracle(kmin, kmax, top_n, big):
    rows, exp = X.expected(kmin, kmax)
    rip = kmin <= 2 <= kmax
    with R.engine(kmin, kmax) as e:
        res = e.explain_ranges(*R.arrays(rows), top_n, rip=rip, big=big)
        ms = e.kernel_ms(7)
        score = e.score_ranges(*R.arrays(rows), rip=rip, big=big)
    assert ms > 0.0
    _same(res, score, SCORE + (["pi", "si", "cri"] if rip else []))
    _, checked, ties, complete = check_explain("explain k=%d..%d top %d %s" % (kmin, kmax, top_n, "big" if big else "auto"), res, exp,
                                            kmax, top_n)
    assert checked >= 60
    if top_n == 64:
        # every length <= 65 has at most 64 max-mers; at kmax = 3 (4^3 = 64) every scored row has a complete list, the long ones too
        assert complete >= (checked if kmax <= 3 else 36)
    if (kmin, kmax) in ((1, 3), (2, 2)):
        full = [r for r, x in enumerate(exp) if x is not None and x["flag"] == H.OK and x["m"] == 4 ** kmax]
        assert len(full) >= 5 and all(int(res.n_present[r]) == 4 ** kmax for r in full)
    if (kmin, kmax, top_n) == (8, 8, 64):
        # ties: at (8, 8) a term depends on the max-mer's count in the range and in the genome alone, so equal counts give bit-equal
        # terms (a CPU probe: 948 exact ties within the top 17 over the set's 82 scored rows) - clause (c)'s tie rule is exercised
        assert ties >= 1, ties


# --------------------------------------------------------------------------------------------------------- orphan hand-over
def test_orphan_hand_over_gives_the_same_bytes():
    """The rows of test_orphan_list_hands_over_to_the_long_form: (2, 0, 650) overflows the LDS list and reaches the long form
    through the device list."""
    rows = [(2, 0, 640), (2, 0, 650), (2, 0, 65535), (2, 10, 650), (0, 100, 700)]
    exp = X.explain_rows(R.scaffolds(), R.profile(1, 8), rows, 1, 8)
    assert all(x is not None and x["flag"] == H.OK for x in exp)
    with R.engine(1, 8) as e:
        auto = e.explain_ranges(*R.arrays(rows), 64, rip=True)
        big = e.explain_ranges(*R.arrays(rows), 64, rip=True, big=True)
    check_explain("explain orphan hand-over", auto, exp, 8, 64)
    assert len(_cols(True)) == 13 and _same(auto, big, _cols(True))


# ---------------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("kmin,kmax", [(1, 8), (1, 6), (2, 9)])
def test_rows_do_not_depend_on_the_call(kmin, kmax):
    import torch
    rows, _ = X.expected(kmin, kmax)
    s, a, b = R.arrays(rows)
    n, top_n, cols = len(rows), 16, _cols(True)
    with R.engine(kmin, kmax) as e:
        scan0 = e.scan(5000, 1000, rip=True)
        score0 = e.score_ranges(s, a, b, rip=True)
        first = e.explain_ranges(s, a, b, top_n, rip=True)
        again = e.explain_ranges(s, a, b, top_n, rip=True)
        perm = np.random.default_rng(5).permutation(n)
        shuffled = e.explain_ranges(s[perm], a[perm], b[perm], top_n, rip=True)
        cut = n // 3
        halves = [e.explain_ranges(s[:cut], a[:cut], b[:cut], top_n, rip=True), e.explain_ranges(s[cut:], a[cut:], b[cut:], top_n, rip=True)]
        copies = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
        one = rows.index((0, 64, 64 + R.T_SHORT + 1))
        many = e.explain_ranges(np.full(copies, s[one]), np.full(copies, a[one]), np.full(copies, b[one]), top_n, rip=True)
        scan1 = e.scan(5000, 1000, rip=True)
        score1 = e.score_ranges(s, a, b, rip=True)
    _same(first, again, cols)
    _same(first, shuffled, cols, ia=perm)
    _same(first, halves[0], cols, ia=np.arange(cut))
    _same(first, halves[1], cols, ia=np.arange(cut, n))
    _same(first, many, cols, ia=np.full(copies, one))
    assert int(first.n_present[one]) > top_n and (first.code[one] != NONE).all()
    assert len(scan0) > 0
    _same(scan0, scan1, ["seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri"])
    _same(score0, score1, SCORE + ["pi", "si", "cri"])
    _same(score0, first, SCORE + ["pi", "si", "cri"])


# --------------------------------------------------------------------------------------------------------------- rejections
def test_rejected_calls_launch_nothing_and_leave_the_state():
    import ctypes
    from frisk_amd import _ffi
    from frisk_amd.engine import Engine
    known = [(0, 64, 64 + 513)]
    exp = X.explain_rows(R.scaffolds(), R.profile(1, 8), known, 1, 8)
    n0 = len(R.scaffolds()[0])

    def code(e, rows, top_n=4, **kw):
        with pytest.raises(_ffi.FriskHipError) as err:
            e.explain_ranges(*R.arrays(rows), top_n, **kw)
        return err.value.code

    def explains(e, tag):
        check_explain(tag, e.explain_ranges(*R.arrays(known), 8, rip=True), exp, 8, 8)

    with Engine(1, 8) as e:
        assert code(e, known) == _ffi.E_ARG                                     # no resident batch
        e.load(R.scaffolds())
        assert code(e, known) == _ffi.E_STATE                                   # no finalised profile
        sym, meta = R.profile(1, 8)
        e.profile_set(sym, *[int(v) for v in meta])
        for bad in ([(4, 0, 10)], [(-1, 0, 10)], [(0, -1, 10)], [(0, 10, 10)], [(0, 10, 9)], [(0, 0, n0 + 1)], [(3, 0, 12)],
                    known + [(0, 5, n0 + 1)]):
            assert code(e, bad) == _ffi.E_ARG, bad
            explains(e, "after a rejected call")
        for top_n in (0, 65, -1):
            assert code(e, known, top_n=top_n) == _ffi.E_ARG, top_n
            explains(e, "after top_n = %d" % top_n)
        e.load_fasta_shard(os.path.join(INPUTS, "markov_islands.fa"), 400, 150, 0, 1)       # a tiled batch
        assert code(e, [(0, 0, 10)]) == _ffi.E_ARG
        e.load(R.scaffolds())
        explains(e, "after a tiled batch")
        # a null required array, one at a time; n = 0 touches nothing
        s, a, b = R.arrays(known)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
        lib = _ffi.lib()
        st, nn, npres = np.zeros(1, np.uint32), np.full(1, -7, np.int64), np.full(1, -7, np.int32)
        d = [np.full(4, -7.0) for _ in range(6)]
        u = [np.full(4, 7, np.uint32) for _ in range(2)]
        full = [p(st), p(d[0]), p(d[1]), None, None, None, p(nn), p(npres), p(u[0]), p(u[1]), p(d[2]), p(d[3]), p(d[4])]
        for hole in (0, 1, 2, 6, 7, 8, 9, 10, 11, 12):                            # status kld gc nn n_present code count pw pg term
            args = list(full)
            args[hole] = None
            assert lib.frisk_explain_ranges(e._ctx, p(s), p(a), p(b), 1, 0, 4, *args) == _ffi.E_ARG, hole
        assert lib.frisk_explain_ranges(e._ctx, p(s), p(a), p(b), 1, _ffi.SCAN_RIP, 4, *full) == _ffi.E_ARG       # pi / si / cri with RIP
        assert lib.frisk_explain_ranges(e._ctx, None, None, None, 0, 0, 4, *([None] * 13)) == _ffi.OK
        assert lib.frisk_explain_ranges(e._ctx, p(s), p(a), p(b), 0, 0, 4, *full) == _ffi.OK
        assert nn[0] == -7 and npres[0] == -7 and all((x == -7.0).all() for x in d) and all((x == 7).all() for x in u)
        explains(e, "after null arrays")
        e.profile_reset()
        assert code(e, known) == _ffi.E_STATE
        e.profile_add(); e.profile_finalize()
        assert len(e.explain_ranges(*R.arrays(known), 8)) == 1
    with Engine(3, 5) as e:                                                     # RIP needs the dinucleotides
        e.load(R.scaffolds())
        sym, meta = R.profile(3, 5)
        e.profile_set(sym, *[int(v) for v in meta])
        assert code(e, known, rip=True) == _ffi.E_ARG
        assert len(e.explain_ranges(*R.arrays(known), 4)) == 1


# ------------------------------------------------------------------------------------------------------------- command line
def _count(text, word):
    return sum(text.startswith(word, i) for i in range(len(text) - len(word) + 1))


def test_command_line_lists_the_kmers_and_leaves_the_score_table(tmp_path):
    from frisk_amd import regions
    fa = os.path.join(INPUTS, "markov_islands.fa")
    seqs = {}
    name = None
    for line in open(fa):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    seqs = {k: "".join(v) for k, v in seqs.items()}
    first = next(iter(seqs))
    n = len(seqs[first])
    bed = tmp_path / "r.bed"
    regs = [(first, 0, 400, "a"), (first, 100, 108, "three"), (first, 0, 3, "short"), (first, n - 900, n, "tail"), (first, 50, 62, "few")]
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % r for r in regs))
    k = 6
    base = ["-H", fa, "-k", str(k), "--bed", str(bed)]
    assert regions.main(base + ["-t", str(tmp_path / "plain")]) == 0
    assert regions.main(base + ["-t", str(tmp_path / "top"), "--topKmers", "5"]) == 0
    plain = (tmp_path / "plain" / "region_scores.tsv").read_bytes()
    assert (tmp_path / "top" / "region_scores.tsv").read_bytes() == plain
    assert not (tmp_path / "plain" / "region_kmers.tsv").exists()
    notes = [l.split("\t")[-1] for l in plain.decode().split("\n")[1:-1]]
    assert notes.count(".") >= 4 and "noMaxmer" in notes
    lines = (tmp_path / "top" / "region_kmers.tsv").read_text().split("\n")
    assert lines[0].split("\t") == regions.KMER_COLUMNS and lines[-1] == ""
    got = {}
    for l in lines[1:-1]:
        f = l.split("\t")
        got.setdefault(f[3], []).append(f)
    assert list(got) == [r[3] for r, note in zip(regs, notes) if note == "."]        # input order, scored regions only
    for (sc, a, b, ident), note in zip(regs, notes):
        if note != ".":
            continue
        text = seqs[sc][a:b].upper()
        present = len({text[i:i + k] for i in range(len(text) - k + 1) if set(text[i:i + k]) <= set("ACGT")})
        rows = got[ident]
        assert [int(f[4]) for f in rows] == list(range(1, min(5, present) + 1)), ident
        terms = [float(f[9]) for f in rows]
        assert terms == sorted(terms, reverse=True)
        for f in rows:
            assert f[:3] == [sc, str(a + 1), str(b)] and len(f[5]) == k and set(f[5]) <= set("ACGT")
            assert int(f[6]) == _count(text, f[5]) >= 1, f
    assert len(got["three"]) <= 3 and len(got["a"]) == 5
    assert regions.main(base + ["-t", str(tmp_path / "null"), "--topKmers", "5", "--null", "markov", "--nullDraws", "8"]) == 0
    assert (tmp_path / "null" / "region_scores.tsv").read_bytes() == plain
    assert (tmp_path / "null" / "region_kmers.tsv").read_text() == "\n".join(lines)
    assert (tmp_path / "null" / "region_null_scores.tsv").read_text().count("\n") == len(regs) + 1
