"""python -m frisk_amd.regions and the C ABI's frisk_score_ranges, as far as a machine without a GPU can tell: the symbol, the
BED / GFF readers and their coordinates, and the module end to end on an engine whose score_ranges is the numpy oracle."""
import ctypes as C
import gzip
import os
import pickle
import re

import numpy as np
import pytest

import ranges_cases as R
from fake_engine import FakeEngine
from oracle import frisk_oracle_np as N

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_score_ranges_symbol_is_declared_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    from frisk_amd import _ffi
    text = open(os.path.join(REPO, "include", "frisk_hip.h")).read()
    m = re.search(r"#define\s+FRISK_RANGES_BIG\s+(0x[0-9a-fA-F]+|\d+)u", text)
    assert m and int(m.group(1), 0) == _ffi.RANGES_BIG
    assert not _ffi.RANGES_BIG & (_ffi.SCAN_RIP | _ffi.SCAN_SCAFFOLDS_ALL | _ffi.SCAN_CHUNKS | _ffi.SCAN_BITS4 | _ffi.SCAN_SIDE4)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+frisk_score_ranges\s*\(\s*frisk_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*seq_index\s*,\s*const\s+int64_t\s*\*\s*"
                     r"start\s*,\s*const\s+int64_t\s*\*\s*stop\s*,\s*int64_t\s+n\s*,\s*uint32_t\s+flags\s*,\s*uint32_t\s*\*\s*status\s*,"
                     r"\s*double\s*\*\s*kld\s*,\s*double\s*\*\s*gc\s*,\s*double\s*\*\s*pi\s*,\s*double\s*\*\s*si\s*,\s*double\s*\*\s*cri\s*,"
                     r"\s*int64_t\s*\*\s*nn\s*\)", text)
    table = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert table["frisk_score_ranges"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_uint32] + [C.c_void_p] * 7)
    lib = _ffi.lib()
    assert lib.frisk_score_ranges(None, None, None, None, 0, 0, None, None, None, None, None, None, None) == _ffi.E_ARG
    assert "frisk_ranges.hip" in g.HIP_SOURCES
    from frisk_amd.engine import Engine
    assert callable(Engine.score_ranges)


@pytest.mark.parametrize("kmin,kmax", R.ORDERS)
def test_range_set_of_the_device_tests_has_its_classes(kmin, kmax):
    """No range is DEGENERATE; four ranges dropped by the N rule (inside the N run, 80 % N, half and all soft-masked), six to
    eight without a max-mer and - at K = 8 and at (2, 9) - one ZeroDivisionError are present, by the oracle's flags."""
    rows, exp = R.expected(kmin, kmax)
    dropped, nomax, zero, degenerate = R.classes(exp)
    assert degenerate == 0 and dropped == 4 and 6 <= nomax <= 8
    assert zero == (1 if kmax >= 8 else 0)
    assert sorted(rows[i] for i, e in enumerate(exp) if e["status"] == 0) == [(0, 1495, 1545), (0, 1505, 1535), (0, 2400, 3000),
                                                                              (0, 2540, 2840)]
    if zero:
        assert [rows[i][0] for i, e in enumerate(exp) if e["status"] & R.ZERO_WEIGHT] == [3]


def test_cli_parser_is_still_the_reference_surface():
    import test_postprocess_cpu as T
    T.test_cli_surface_equals_reference()


# --------------------------------------------------------------------------------------------------------------- readers
def test_bed_reader_coordinates_ids_and_skipped_lines(tmp_path):
    from frisk_amd import regions
    text = ("# a comment\ntrack name=x\nbrowser position chr1:1-10\n\nchr1\t0\t1\tfirst\r\nchr1\t199\t200\n"
            "chr2\t5\t50\tg1\t0\t+\nchr1\t7\t9\t\n")
    plain = tmp_path / "a.bed"
    plain.write_bytes(text.encode())
    want = [("chr1", 0, 1, "first"), ("chr1", 199, 200, "."), ("chr2", 5, 50, "g1"), ("chr1", 7, 9, ".")]
    assert regions.read_bed(str(plain)) == want
    gz = tmp_path / "a.bed.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(text.replace("\n", "\r\n").replace("\r\r\n", "\r\n").encode())
    assert regions.read_bed(str(gz)) == want
    for bad in ("chr1\t5\n", "chr1\ta\t9\n", "chr1\t9\t9\n", "chr1\t-1\t9\n"):
        p = tmp_path / "bad.bed"
        p.write_text("chr1\t0\t5\n" + bad)
        with pytest.raises(ValueError, match="line 2"):
            regions.read_bed(str(p))


def test_gff_reader_is_one_based_inclusive_and_takes_the_id(tmp_path):
    from frisk_amd import regions
    text = ("##gff-version 3\nchr1\tsrc\tgene\t1\t1\t.\t+\t.\tID=first;Name=a\r\nchr1\tsrc\tmRNA\t5\t80\t.\t+\t.\tParent=first\n"
            "chr1\tsrc\tgene\t200\t200\t.\t-\t.\tName=b; ID=last\nchr2\tsrc\tgene\t10\t19\t.\t+\t.\t.\n")
    p = tmp_path / "a.gff3"
    p.write_bytes(text.encode())
    assert regions.read_gff_regions(str(p)) == [("chr1", 0, 1, "first"), ("chr1", 4, 80, "."), ("chr1", 199, 200, "last"),
                                                ("chr2", 9, 19, ".")]
    assert regions.read_gff_regions(str(p), ["gene"]) == [("chr1", 0, 1, "first"), ("chr1", 199, 200, "last"), ("chr2", 9, 19, ".")]
    gz = tmp_path / "a.gff3.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(text.encode())
    assert regions.read_gff_regions(str(gz), ["mRNA"]) == [("chr1", 4, 80, ".")]


def test_regions_parser_takes_the_main_options_and_exactly_one_source():
    from frisk_amd import cli, regions
    main = {a.dest: a for a in cli.build_parser()._actions}
    mine = {a.dest: a for a in regions.build_parser()._actions}
    for dest in ("hostSeq", "querySeq", "minWordSize", "maxWordSize", "tempDir", "maskHost", "recalc", "RIP"):
        a, b = main[dest], mine[dest]
        assert (a.option_strings, a.default, type(a), a.type, a.required) == (b.option_strings, b.default, type(b), b.type, b.required), dest
    assert mine["outfile"].option_strings == ["-O", "--outfile"] and mine["outfile"].default == "region_scores.tsv"
    parse = regions.build_parser().parse_args
    assert parse(["-H", "h.fa", "--bed", "x.bed"]).recalc is True and parse(["-H", "h.fa", "--bed", "x.bed", "--recalc"]).recalc is False
    assert parse(["-H", "h.fa", "--gff", "x.gff", "--gffFeatures", "gene", "mRNA"]).gffFeatures == ["gene", "mRNA"]
    for argv in (["-H", "h.fa"], ["-H", "h.fa", "--bed", "a", "--gff", "b"]):
        with pytest.raises(SystemExit):
            parse(argv)


# ------------------------------------------------------------------------------------------ the module on an oracle engine
class _Engine(FakeEngine):
    """FakeEngine with the members of Engine that HotPath.scoreRegions touches; score_ranges is the numpy oracle."""
    adds = 0

    def __init__(self, kmin, kmax, device=0):
        super().__init__(kmin, kmax)
        self.tiles = None

    @property
    def seq_lens(self):
        return [e.n for e in self.seqs]

    def profile_add(self, *a, **k):
        _Engine.adds += 1
        return super().profile_add(*a, **k)

    def profile_set(self, sym, tl, ex, nn):
        self.profile = (np.asarray(sym, dtype=np.int64), (tl, ex, nn))

    def close(self):
        pass

    def score_ranges(self, seq_index, start, stop, rip=False, big=False):
        from frisk_amd.engine import ScanResult
        sym, meta = self.profile
        ig = N.genome_ivom_table(sym, meta, self.kmin, self.kmax)
        rows = list(zip(np.asarray(seq_index).tolist(), np.asarray(start).tolist(), np.asarray(stop).tolist()))
        exp = R.expect_rows(self.seqs, self.profile, ig, rows, self.kmin, self.kmax)
        nan = float("nan")
        kld = [float(e["kld_hp"]) if e["flag"] == 0 else (0.0 if e["flag"] == 8 else nan) for e in exp]
        col = lambda i: np.array([e["rip"][i] if e["rip"] else nan for e in exp]) if rip else None      # noqa: E731
        return ScanResult(seq_index=np.asarray(seq_index), start=np.asarray(start), stop=np.asarray(stop),
                          status=np.array([e["status"] for e in exp], np.uint32), kld=np.array(kld), gc=np.array([e["gc"] for e in exp]),
                          pi=col(0), si=col(1), cri=col(2), nn=np.array([e["nn"] for e in exp], np.int64))


@pytest.fixture
def fake_regions(monkeypatch):
    from frisk_amd import hotpath, regions
    monkeypatch.setattr(hotpath, "Engine", _Engine)
    real_init = hotpath.HotPath.__init__

    def init(self, kMin, kMax, device=0, cache_dir=None, use_cache=True):
        real_init(self, kMin, kMax, device=device, cache_dir=None, use_cache=use_cache)      # (no packed-sequence cache: no device)
    monkeypatch.setattr(hotpath.HotPath, "__init__", init)
    _Engine.adds = 0
    return regions


def _inputs(tmp_path):
    rng = np.random.default_rng(3)
    rnd = lambda n: R._bases(rng, n, 0.5).decode()        # noqa: E731
    chr1 = rnd(120) + "N" * 30 + rnd(50)
    fa = tmp_path / "g.fa"
    fa.write_text(">chr1 the first\n%s\n%s\n>tiny\nACGTTGCAacg\n" % (chr1[:70], chr1[70:]))
    bed = tmp_path / "r.bed"
    bed.write_text("tiny\t5\t9\tzw\nchr1\t0\t100\tgeneA\nchr1\t115\t155\tgap\nchr1\t0\t3\nchr1\t199\t200\tlastbase\nchr1\t0\t1\tfirstbase\n")
    return str(fa), str(bed), chr1


def _gc(s):
    up = [c for c in s if c in "ACGT"]
    return sum(c in "GC" for c in up) / float(len(up))


def test_module_end_to_end_table_text_order_and_cache(fake_regions, tmp_path, caplog):
    from frisk_amd import postprocess as pp
    fa, bed, chr1 = _inputs(tmp_path)
    out = tmp_path / "t"
    argv = ["-H", fa, "-k", "4", "-t", str(out), "--bed", bed]
    assert fake_regions.main(argv) == 0
    lines = (out / "region_scores.tsv").read_text().split("\n")
    assert lines[0] == "name\tstart\tstop\tlength\twindowKLD\tGC\tid\tnote" and lines[-1] == "" and len(lines) == 8
    # the scored row: its numbers from the oracle on the slice, its text from the score table's formatter
    enc = N.Encoded(chr1[:100])
    prof = N.genome_profile([chr1, "ACGTTGCAacg"], 1, 4)
    kld = N.score_window(enc, N.genome_ivom_table(prof[0], prof[1], 1, 4), 1, 4)["KLD"]
    assert lines[2].split("\t")[:4] == ["chr1", "1", "100", "100"] and lines[2].split("\t")[6:] == ["geneA", "."]
    assert abs(float(lines[2].split("\t")[4]) - kld) <= 1e-11 and lines[2].split("\t")[5] == pp.py2_str(_gc(chr1[:100]))
    # one row of each other note, written by hand; input order kept
    assert lines[1] == "tiny\t6\t9\t4\tnan\t0.666666666667\tzw\tZeroDivisionError"       # GCAa: S = 3 = kmax - 1, the max-mer GCAA
    assert lines[3] == "chr1\t116\t155\t40\tnan\tnan\tgap\tunresolved"                   # 30 N of 40
    assert lines[4] == "chr1\t1\t3\t3\t0\t%s\t.\tnoMaxmer" % pp.py2_str(_gc(chr1[:3]))
    assert lines[5] == "chr1\t200\t200\t1\t0\t%s\tlastbase\tnoMaxmer" % pp.py2_str(_gc(chr1[199:]))
    assert lines[6] == "chr1\t1\t1\t1\t0\t%s\tfirstbase\tnoMaxmer" % pp.py2_str(_gc(chr1[:1]))
    # the genome cache file of the main command line: written by the first run, read by the second
    cache = out / "g.fa_kmers_1_4_genome.p"
    assert cache.is_file() and _Engine.adds == 1
    with open(cache, "rb") as fh:
        maps = pickle.load(fh)
    assert maps[-3] == {"totalLen": 211} and len(maps) == 4 + 3
    first = (out / "region_scores.tsv").read_text()
    assert fake_regions.main(argv + ["--RIP"]) == 0 and _Engine.adds == 1
    rip = (out / "region_scores.tsv").read_text().split("\n")
    assert rip[0] == "name\tstart\tstop\tlength\twindowKLD\tGC\tPI\tSI\tCRI\tid\tnote"
    assert [l.split("\t")[:6] + l.split("\t")[9:] for l in rip[1:-1]] == [l.split("\t") for l in first.split("\n")[1:-1]]
    want = N.score_window(enc, N.genome_ivom_table(prof[0], prof[1], 1, 4), 1, 4, rip=True)["RIP"]
    assert rip[2].split("\t")[6:9] == [pp.py2_str(float(v)) for v in want]
    assert rip[3].split("\t")[6:9] == ["nan"] * 3
    # --recalc (store_false) forces the profile again
    assert fake_regions.main(argv + ["--recalc", "-O", "again.tsv"]) == 0 and _Engine.adds == 2
    assert (out / "again.tsv").read_text() == first


def test_module_with_a_gff_and_a_query(fake_regions, tmp_path):
    fa, _bed, chr1 = _inputs(tmp_path)
    host = tmp_path / "h.fa"
    host.write_text(">h\n%s\n" % (chr1[:120] * 3))
    gff = tmp_path / "r.gff3"
    gff.write_text("chr1\ts\tgene\t1\t100\t.\t+\t.\tID=g1\nchr1\ts\texon\t1\t50\t.\t+\t.\tID=e1\nchr1\ts\tgene\t200\t200\t.\t+\t.\tNote=x\n")
    out = tmp_path / "t"
    assert fake_regions.main(["-H", str(host), "-Q", fa, "-k", "4", "-t", str(out), "--gff", str(gff), "--gffFeatures", "gene"]) == 0
    lines = (out / "region_scores.tsv").read_text().split("\n")
    assert [l.split("\t")[:4] + l.split("\t")[6:] for l in lines[1:-1]] == [["chr1", "1", "100", "100", "g1", "."],
                                                                          ["chr1", "200", "200", "1", ".", "noMaxmer"]]
    assert (out / "h.fa_kmers_1_4_genome.p").is_file()
    prof = N.genome_profile([chr1[:120] * 3], 1, 4)
    kld = N.score_window(N.Encoded(chr1[:100]), N.genome_ivom_table(prof[0], prof[1], 1, 4), 1, 4)["KLD"]
    assert abs(float(lines[1].split("\t")[4]) - kld) <= 1e-11


def test_module_refuses_unknown_scaffolds_and_overruns_and_takes_an_empty_input(fake_regions, tmp_path, caplog):
    fa, _bed, _ = _inputs(tmp_path)
    out = tmp_path / "t"
    for text, word in (("chr1\t0\t50\tok\nchr9\t0\t50\tnope\n", "region 2 (chr9:1-50)"), ("chr1\t150\t201\tover\n", "region 1 (chr1:151-201)")):
        bed = tmp_path / "bad.bed"
        bed.write_text(text)
        caplog.clear()
        assert fake_regions.main(["-H", fa, "-k", "4", "-t", str(out), "--bed", str(bed)]) == 1
        assert word in caplog.text
        assert not (out / "region_scores.tsv").exists()
    empty = tmp_path / "empty.bed"
    empty.write_text("# nothing\ntrack name=none\n")
    assert fake_regions.main(["-H", fa, "-k", "4", "-t", str(out), "--bed", str(empty), "--RIP"]) == 0
    assert (out / "region_scores.tsv").read_text() == "name\tstart\tstop\tlength\twindowKLD\tGC\tPI\tSI\tCRI\tid\tnote\n"
