"""frisk_explain_ranges and python -m frisk_amd.regions --topKmers, as far as a machine without a GPU can tell: the symbol, the
calibration of the per-term bound, the command line's checks, the k-mer text and the row writer on a fabricated result, and the
oracle's own sums."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import explain_oracle as X
import kld_oracle_hp as H
import ranges_cases as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_explain_ranges_symbol_is_declared_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    from frisk_amd import _ffi
    text = open(os.path.join(REPO, "include", "frisk_hip.h")).read()
    m = re.search(r"#define\s+FRISK_EXPLAIN_MAX\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _ffi.EXPLAIN_MAX == 64
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ptr = lambda t, n: r"\s*%s\s*\*\s*%s\s*" % (t.replace(" ", r"\s+"), n)                    # noqa: E731
    args = [ptr("frisk_ctx", "ctx"), ptr("const int32_t", "seq_index"), ptr("const int64_t", "start"), ptr("const int64_t", "stop"),
            r"\s*int64_t\s+n\s*", r"\s*uint32_t\s+flags\s*", r"\s*int32_t\s+top_n\s*", ptr("uint32_t", "status"), ptr("double", "kld"),
            ptr("double", "gc"), ptr("double", "pi"), ptr("double", "si"), ptr("double", "cri"), ptr("int64_t", "nn"),
            ptr("int32_t", "n_present"), ptr("uint32_t", "code"), ptr("uint32_t", "count"), ptr("double", "pw"), ptr("double", "pg"),
            ptr("double", "term")]
    assert re.search(r"\bint\s+frisk_explain_ranges\s*\(" + ",".join(args) + r"\)\s*;", text)
    table = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert table["frisk_explain_ranges"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_uint32, C.c_int32] + [C.c_void_p] * 13)
    lib = _ffi.lib()
    assert lib.frisk_explain_ranges(None, None, None, None, 0, 0, 1, *([None] * 13)) == _ffi.E_ARG
    assert "frisk_ranges.hip" in g.HIP_SOURCES and "explain_kernels.h" in open(os.path.join(g.CSRC, "frisk_ranges.hip")).read()
    from frisk_amd.engine import Engine
    from frisk_amd.hotpath import HotPath
    assert callable(Engine.explain_ranges) and callable(HotPath.explainRegions)


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_c_term_is_calibrated_and_the_oracle_terms_sum_to_the_kld():
    """C_TERM is the smallest power of two at least four times the worst normalised term error of the two FP64 restatements over
    the scored rows of the range set at every order; the s_k of a row add up to its scale and the t_k to its KLD."""
    cal = X.calibration()
    for (kmin, kmax), (two, one, n) in cal.items():
        print("term calibration k=%d..%d: worst normalised error two-pass %.2f, one-pass %.2f over %d rows" % (kmin, kmax, two, one, n))
    overall = max(max(two, one) for two, one, _ in cal.values())
    print("C_TERM = %g (smallest power of two >= 4 x %.2f)" % (X.C_TERM, overall))
    assert all(n >= 60 for _, _, n in cal.values()), cal
    assert X.C_TERM == 2.0 ** math.ceil(math.log2(4 * overall)), (X.C_TERM, overall)
    checked = 0
    for kmin, kmax in R.ORDERS:
        _rows, exp = X.expected(kmin, kmax)
        for e in exp:
            if e is None or e["flag"] != H.OK:
                continue
            assert e["count"].sum() > 0 and e["present"].size == e["m"] == e["t_hp"].size
            assert abs(e["t_hp"].sum() - e["kld"]) <= 4 * np.finfo(H.LD).eps * e["scale"] * e["m"]
            assert abs(float(e["s"].sum()) - e["scale"]) <= 1e-12 * e["scale"]
            checked += 1
    assert checked >= 400


def test_oracle_rows_are_those_of_the_score_oracle():
    """The same rows dropped, the same flags and the same extended-precision KLD as ranges_cases.expected."""
    for kmin, kmax in [(1, 8), (3, 5)]:
        rows, exp = R.expected(kmin, kmax)
        rows2, mine = X.expected(kmin, kmax)
        assert rows == rows2
        for e, m in zip(exp, mine):
            assert (e["status"] == 0) == (m is None)
            if m is not None:
                assert e["flag"] == m["flag"] and e["kld_hp"] == m["kld"]


# ---------------------------------------------------------------------------------------------------------- command line
def test_parser_knows_the_options_and_refuses_bad_values(tmp_path, caplog):
    from frisk_amd import regions
    mine = {a.dest: a for a in regions.build_parser()._actions}
    assert mine["topKmers"].option_strings == ["--topKmers"] and mine["topKmers"].default is None and mine["topKmers"].type is int
    assert mine["kmerOutfile"].option_strings == ["--kmerOutfile"] and mine["kmerOutfile"].default == "region_kmers.tsv"
    bed = tmp_path / "r.bed"
    bed.write_text("chr1\t0\t50\n")
    base = ["-H", str(tmp_path / "absent.fa"), "-t", str(tmp_path / "t"), "--bed", str(bed)]
    for extra, word in ((["--topKmers", "0"], "1..64"), (["--topKmers", "65"], "1..64"), (["--topKmers", "-3"], "1..64"),
                        (["--topKmers", "5", "--donors", str(tmp_path / "d.fa")], "--donors")):
        caplog.clear()
        assert regions.main(base + extra) == 1          # (before any device work: the host FASTA does not even exist)
        assert word in caplog.text
        assert not (tmp_path / "t").exists()
    args = regions.build_parser().parse_args(base + ["--topKmers", "64", "--null", "markov"])
    assert regions.kmers_problem(args) is None and regions.null_problem(args, [("chr1", 0, 50, ".")]) is None


def test_an_empty_region_list_writes_the_header_only(tmp_path):
    from frisk_amd import regions
    bed = tmp_path / "empty.bed"
    bed.write_text("# nothing\n")
    out = tmp_path / "t"
    assert regions.main(["-H", str(tmp_path / "absent.fa"), "-t", str(out), "--bed", str(bed), "--topKmers", "3"]) == 0
    assert (out / "region_kmers.tsv").read_text() == "name\tstart\tstop\tid\trank\tkmer\tcount\tpw\tpg\tterm\tshare\n"
    assert (out / "region_scores.tsv").read_text().count("\n") == 1


def test_kmer_text_is_the_tables_digit_order():
    from frisk_amd.regions import kmer_text
    assert kmer_text(0, 8) == "AAAAAAAA" and kmer_text(1, 8) == "AAAAAAAT" and kmer_text(0xFFFF, 8) == "CCCCCCCC"
    assert kmer_text(2, 1) == "G" and kmer_text(0b00011011, 4) == "ATGC" and kmer_text(np.uint32(3 << 22), 12) == "C" + "A" * 11


def test_row_writer_on_a_fabricated_result():
    from frisk_amd import _ffi, regions
    from frisk_amd import postprocess as pp
    from frisk_amd.engine import ScanResult
    nan = float("nan")
    none = _ffi.EXPLAIN_NONE
    regs = [("c", 0, 100, "a"), ("c", 5, 9, "."), ("c", 10, 90, "zw"), ("c", 0, 3, "nm"), ("c", 20, 60, "zero"), ("c", 30, 70, "one")]
    res = ScanResult(
        status=np.array([1, 0, 3, 9, 1, 1], np.uint32), kld=np.array([0.5, nan, nan, 0.0, 0.0, 0.25]),
        n_present=np.array([5, 0, 7, 0, 2, 1], np.int32),
        code=np.array([[27, 0, 255], [none] * 3, [none] * 3, [none] * 3, [1, 2, none], [228, none, none]], np.uint32),
        count=np.array([[3, 1, 2], [0] * 3, [0] * 3, [0] * 3, [1, 1, 0], [4, 0, 0]], np.uint32),
        pw=np.array([[0.25, 0.125, 0.5], [nan] * 3, [nan] * 3, [nan] * 3, [0.5, 0.5, nan], [1.0, nan, nan]]),
        pg=np.array([[0.125, 0.125, 0.75], [nan] * 3, [nan] * 3, [nan] * 3, [0.25, 1.0, nan], [0.5, nan, nan]]),
        term=np.array([[0.75, 0.0, -0.125], [nan] * 3, [nan] * 3, [nan] * 3, [0.5, -0.5, nan], [0.25, nan, nan]]))
    lines = list(regions.kmer_rows(regs, res, 4, pp.py2_str))
    assert lines == [
        "c\t1\t100\ta\t1\tATGC\t3\t0.25\t0.125\t0.75\t1.5\n",
        "c\t1\t100\ta\t2\tAAAA\t1\t0.125\t0.125\t0.0\t0.0\n",
        "c\t1\t100\ta\t3\tCCCC\t2\t0.5\t0.75\t-0.125\t-0.25\n",       # min(N, present): three slots of five max-mers
        "c\t21\t60\tzero\t1\tAAAT\t1\t0.5\t0.25\t0.5\t.\n",          # a KLD of 0: no share
        "c\t21\t60\tzero\t2\tAAAG\t1\t0.5\t1.0\t-0.5\t.\n",
        "c\t31\t70\tone\t1\tCGTA\t4\t1.0\t0.5\t0.25\t1.0\n"]         # (unresolved, ZeroDivisionError, noMaxmer: no lines)
    assert regions.KMER_COLUMNS == "name start stop id rank kmer count pw pg term share".split()
    assert "negative" in regions.__doc__ and "--topKmers" in regions.__doc__
