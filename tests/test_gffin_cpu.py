"""--gffIn without a GPU: `bedtools window -w W -u` restated (frisk_amd.postprocess.read_gff / window_u / featuresNear) on the
hand-transcribed cases of tests/golden/bedtools_window_semantics.json and against a brute-force loop, the GFF reader, and the CLI
on an oracle-backed engine (reference L1709-1747)."""
import gzip
import json
import logging
import os

import numpy as np
import pytest

import gffin_cases as GC
from frisk_amd import postprocess as pp
from test_update_hmm_cpu import fake_cli  # noqa: F401 - the fixture: the CLI on the oracle-backed engine

WINDOW = json.load(open(os.path.join(GC.GOLD, "bedtools_window_semantics.json")))


# ------------------------------------------------------------------------------------------------------ the recorded cases
def test_golden_names_what_it_is_and_covers_the_listed_cases():
    prov = WINDOW["provenance"]
    assert "transcribed" in prov and "bedtools window" in prov and "not output of a program" in prov
    assert "`-w`" in prov and "`-u`" in prov and "shifted by one" in prov
    names = " | ".join(c["name"] for c in WINDOW["cases"])
    for key in ("book-ended", "w = 0", "w = 1", "minus-one", "clipping at 0", "two regions", "another chrom", "absent from B",
                "nested and unsorted", "type filter", "larger than the scaffold"):
        assert key in names, key


@pytest.mark.parametrize("case", WINDOW["cases"], ids=lambda c: c["name"][:40])
def test_window_u_on_the_recorded_cases(case):
    rows = [ln.split("\t") for ln in case["gff"]]
    rows = [(ln, f) for ln, f in zip(case["gff"], rows) if f[2] in case["feature_types"]]
    reg = case["regions"]
    mask = pp.window_u([f[0] for _l, f in rows], [int(f[3]) - 1 for _l, f in rows], [int(f[4]) for _l, f in rows],
                       [r[0] for r in reg], [r[1] for r in reg], [r[2] for r in reg], case["w"])
    assert mask.dtype == bool and mask.shape == (len(rows),)
    assert [ln for (ln, _f), m in zip(rows, mask.tolist()) if m] == case["expected"]


@pytest.mark.parametrize("case", WINDOW["cases"], ids=lambda c: c["name"][:40])
def test_featuresNear_on_the_recorded_cases(case, tmp_path):
    path = tmp_path / "a.gff"
    path.write_text("##gff-version 3\n" + "".join(ln + "\n" for ln in case["gff"]))
    recs = pp.read_gff(str(path), case["feature_types"])
    assert pp.featuresNear(recs, [tuple(r) for r in case["regions"]], case["w"]) == [ln + "\n" for ln in case["expected"]]
    # regions as a generator, with further fields and numbers as text: the same
    assert pp.featuresNear(recs, ((r[0], str(r[1]), str(r[2]), "0.5") for r in case["regions"]), case["w"]) == \
        [ln + "\n" for ln in case["expected"]]


# ------------------------------------------------------------------------------------------------------ against brute force
def test_window_u_equals_the_brute_force_loop_on_every_random_case():
    touching = one_base = kept = dropped = empty_b = 0
    for no in range(GC.RANDOM_CASES):
        a, b, w = GC.random_case(no)
        want = GC.brute_mask(a, b, w)
        got = pp.window_u([r[0] for r in a], [r[1] for r in a], [r[2] for r in a],
                          [r[0] for r in b], [r[1] for r in b], [r[2] for r in b], w)
        assert got.dtype == bool and got.tolist() == want, (no, w)
        kept += sum(want)
        dropped += len(want) - sum(want)
        empty_b += not b
        for ac, a0, a1 in a:
            lo, hi = max(0, a0 - w), a1 + w
            for bc, b0, b1 in b:
                if bc == ac:
                    touching += hi == b0 or lo == b1
                    one_base += min(hi, b1) - max(lo, b0) == 1
    # the cases are what they claim to be: a book-ended pair and a one-base overlap per case on average, both answers in their
    # thousands, an empty B among them
    assert touching > 200 and one_base > 200 and kept > 1000 and dropped > 1000 and empty_b > 0, \
        (touching, one_base, kept, dropped, empty_b)


def test_window_u_edges():
    none = pp.window_u(["c1", "c2"], [0, 5], [10, 6], [], [], [], 100)
    assert none.dtype == bool and none.tolist() == [False, False]                       # empty B
    assert pp.window_u([], [], [], ["c1"], [0], [10], 0).shape == (0,)                  # empty A
    big = 10 ** 30                                                                      # a range no int64 holds
    assert pp.window_u(["c1", "c2"], [0, 5], [10, 6], ["c1"], [10 ** 12], [10 ** 12 + 1], big).tolist() == [True, False]
    with pytest.raises(ValueError):
        pp.window_u(["c1"], [0], [10], ["c1"], [0], [10], -1)
    with pytest.raises(ValueError):
        pp.window_u(["c1"], [0, 1], [10, 11], ["c1"], [0], [10], 0)


# -------------------------------------------------------------------------------------------------------------- read_gff
GENE = "c1\tsrc\tgene\t11\t20\t.\t+\t.\tID=g1"
MRNA = "c1\tsrc\tmRNA\t11\t20\t.\t+\t.\tID=g1.t1;Parent=g1"
EXON = "c2\tsrc\texon\t5\t5\t.\t-\t.\tID=e1"


def test_read_gff_comments_blank_lines_crlf_and_gzip(tmp_path):
    text = "\r\n".join(["##gff-version 3", "# a comment", "", "track name=genes", "browser position c1:1-100", GENE, "   ", MRNA,
                        "###", EXON, "##FASTA", ">c1", "ACGT"]) + "\r\n"
    plain, packed, unix = tmp_path / "a.gff3", tmp_path / "b.gff3.gz", tmp_path / "c.gff3"
    plain.write_bytes(text.encode())
    with gzip.open(packed, "wb") as fh:
        fh.write(text.encode())
    unix.write_bytes(text.replace("\r\n", "\n").encode())
    for path in (plain, packed, unix):
        recs = pp.read_gff(str(path))
        assert len(recs) == 3 and recs.lines == [GENE + "\n", MRNA + "\n", EXON + "\n"]           # written back with "\n" alone
        assert recs.chrom.tolist() == ["c1", "c1", "c2"]
        assert recs.start.tolist() == [10, 10, 4] and recs.end.tolist() == [20, 20, 5]          # [start - 1, end)
        assert recs.start.dtype == recs.end.dtype == np.int64
    # gzip by its magic, not by its name
    odd = tmp_path / "packed.gff3"
    odd.write_bytes(packed.read_bytes())
    assert pp.read_gff(str(odd)).lines == [GENE + "\n", MRNA + "\n", EXON + "\n"]
    empty = tmp_path / "empty.gff3"
    empty.write_text("##gff-version 3\n")
    recs = pp.read_gff(str(empty), ["gene"])
    assert len(recs) == 0 and pp.featuresNear(recs, [("c1", 0, 10)], 5) == []


@pytest.mark.parametrize("bad, word", [("c1\tsrc\tgene\tx11\t20\t.\t+\t.\tID=g", "integers"),
                                       ("c1\tsrc\tgene\t11\t2e1\t.\t+\t.\tID=g", "integers"),
                                       ("c1\tsrc\tgene\t11\t20\t.\t+\t.", "8 tab-separated"),
                                       ("c1 src gene 11 20 . + . ID=g", "1 tab-separated"),
                                       ("c1\tsrc\tgene\t21\t20\t.\t+\t.\tID=g", "behind")])
def test_read_gff_names_the_bad_line(tmp_path, bad, word):
    path = tmp_path / "bad.gff3"
    path.write_text("\n".join(["##gff-version 3", GENE, "", bad, MRNA]) + "\n")
    for types in (None, ["exon"]):              # a malformed line is an error whether or not its type is asked for
        with pytest.raises(ValueError) as err:
            pp.read_gff(str(path), types)
        assert str(path) in str(err.value) and "line 4" in str(err.value) and word in str(err.value)


def test_read_gff_type_filter_is_pythons_in(tmp_path):
    path = tmp_path / "a.gff3"
    path.write_text("\n".join([GENE, MRNA, EXON, GENE.replace("gene", "gen"), GENE.replace("gene", "State1")]) + "\n")
    kinds = lambda recs: [ln.split("\t")[2] for ln in recs.lines]       # noqa: E731
    assert kinds(pp.read_gff(str(path), ["gene"])) == ["gene"]                                      # a list: membership
    assert kinds(pp.read_gff(str(path), ["exon", "gene"])) == ["gene", "exon"]                      # file order
    assert kinds(pp.read_gff(str(path), ("mRNA",))) == ["mRNA"]
    assert kinds(pp.read_gff(str(path), "State1")) == ["State1"]                                    # a string: as `rec[2] in 'State1'`
    assert kinds(pp.read_gff(str(path), "gene")) == ["gene", "gen"]
    assert kinds(pp.read_gff(str(path), [])) == []
    # gffRegions applies the same test to records with GFF numbers and hands out BED numbers
    states = [("s1", "1", "400", "State1"), ("s1", "251", "900", "State2"), ("s2", "1", "50", "State1")]
    assert pp.gffRegions(states, "State1") == [("s1", 0, 400), ("s2", 0, 50)]
    assert pp.gffRegions(states, "State2") == [("s1", 250, 900)]


# ------------------------------------------------------------------------------------------------ the CLI on a fake engine
BASE = ["-H", GC.FASTA, "-m", "2", "-k", "4", "-w", "400", "-i", "150", "-F", "0.08", "--gffOutfile", "a.gff3",
        "--hmmOutfile", "states.gff3", "--RIP", "--minCRI=-1.0", "--peakCRI=0.0", "--minPI=0.8", "--maxSI=1.2"]
ANOM = "featuresIn_thresholded_Anomalies_markov_islands.gff3"
STATE1, STATE2 = "featuresIn_hmm_State1_markov_islands.gff3", "featuresIn_hmm_State2_markov_islands.gff3"
# the anomalies of BASE on this FASTA are chrA 1501-2350, chrA 3001-3550, chrB 151-550 and chrB 1651-2050 (asserted below);
# as BED records with those numbers, the genes of the annotation within 0 / 1 / 10 / 300 bases of one, worked out by hand:
GENES_NEAR = {0: ["gA03", "gA04", "gA05", "gA08", "gB02", "gB05"],
              1: ["gA02", "gA03", "gA04", "gA05", "gA06", "gA08", "gB01", "gB02", "gB05"],
              10: ["gA02", "gA03", "gA04", "gA05", "gA06", "gA08", "gB01", "gB02", "gB03", "gB05"],
              300: ["gA02", "gA03", "gA04", "gA05", "gA06", "gA07", "gA08", "gB01", "gB02", "gB03", "gB05"]}


def _run(cli, tmp_path, sub, extra):
    out = tmp_path / sub
    assert cli.main(BASE + ["-t", str(out)] + extra) == 0
    return out


def _ids(path):
    return [f[8].split(";")[0][3:] for _line, f in GC.gff_rows(path)]


def _messages(caplog):
    return [r.getMessage() for r in caplog.records]


@pytest.mark.parametrize("w", sorted(GENES_NEAR))
def test_cli_anomalies_file_holds_exactly_the_expected_lines(fake_cli, tmp_path, caplog, w):  # noqa: F811
    cli, _made = fake_cli
    with caplog.at_level(logging.INFO, logger="frisk"):
        out = _run(cli, tmp_path, "A", ["--gffIn", GC.GFF, "--gffFeatures", "gene"] + (["--gffRange", str(w)] if w else []))
    anomalies = [(f[0], int(f[3]), int(f[4])) for _line, f in GC.gff_rows(out / "a.gff3")]     # BED: the numbers as they are
    assert anomalies == [("chrA", 1501, 2350), ("chrA", 3001, 3550), ("chrB", 151, 550), ("chrB", 1651, 2050)]
    got = open(out / ANOM, newline="").read()
    assert _ids(out / ANOM) == GENES_NEAR[w]
    assert got == "".join(GC.expected_lines(["gene"], anomalies, w))                          # original lines, input order
    assert not os.path.exists(out / STATE1) and not os.path.exists(out / STATE2)               # no --hmmKLD
    assert "Successfully extracted %d features from within %dbp of anomaly annotations." % (len(GENES_NEAR[w]), w) in _messages(caplog)
    ranges = sorted(GENES_NEAR)
    if w != ranges[0]:                                                                         # a larger range keeps a superset
        smaller = GENES_NEAR[ranges[ranges.index(w) - 1]]
        assert set(smaller) < set(GENES_NEAR[w])


def test_cli_several_types_keep_file_order(fake_cli, tmp_path):  # noqa: F811
    cli, _made = fake_cli
    out = _run(cli, tmp_path, "T", ["--gffIn", GC.GFF, "--gffFeatures", "tRNA", "exon", "gene"])
    assert _ids(out / ANOM) == ["gA03", "gA04", "gA04.t1.e1", "gA04.t1.e2", "gA05", "tA01", "gA08", "gB02", "gB05"]


def test_cli_hmm_adds_the_two_state_files(fake_cli, tmp_path, caplog):  # noqa: F811
    cli, _made = fake_cli
    with caplog.at_level(logging.INFO, logger="frisk"):
        out = _run(cli, tmp_path, "H", ["--hmmKLD", "--gffIn", GC.GFF, "--gffFeatures", "gene", "--gffRange", "10"])
    assert _ids(out / ANOM) == GENES_NEAR[10]
    states = GC.gff_rows(out / "states.gff3")
    assert {f[2] for _line, f in states} == {"State1", "State2"}
    n_genes = len(GC.expected_lines(["gene"], [(c, 0, 10 ** 9) for c in ("chrA", "chrB", "chrM")], 0))
    for name, state in ((STATE1, "State1"), (STATE2, "State2")):
        regions = GC.gff_as_bed(states, [state])                                               # GFF records: [start - 1, end)
        kept = GC.gff_rows(out / name)
        # every kept line lies within range of a state interval, and every line that does is kept, in input order
        assert all(GC.brute_mask(GC.gff_as_bed(kept), regions, 10))
        assert open(out / name, newline="").read() == "".join(GC.expected_lines(["gene"], regions, 10))
        assert 0 < len(kept) < n_genes and {f[2] for _line, f in kept} == {"gene"}
        assert "Successfully extracted %d features from within 10bp of %s hmm annotations." % (len(kept), state) in _messages(caplog)
    assert "gM01" not in _ids(out / STATE1) and "gA09" in _ids(out / STATE1)
    assert _ids(out / STATE2) == ["gA02", "gA03", "gA04"]           # State2 is chrA 1501-1900: [1500, 1900) takes gA02's last base


def test_cli_writes_no_file_when_nothing_is_kept(fake_cli, tmp_path, caplog):  # noqa: F811
    cli, _made = fake_cli
    with caplog.at_level(logging.INFO, logger="frisk"):
        out = _run(cli, tmp_path, "N", ["--hmmKLD", "--gffIn", GC.GFF, "--gffFeatures", "repeat_region"])
    assert sorted(f for f in os.listdir(out) if f.startswith("featuresIn_")) == [STATE1]        # chrB is State1 throughout
    msgs = _messages(caplog)
    assert "No features from %s detected within 0 bases of anomalies." % GC.GFF in msgs
    assert "No features from %s detected within 0 bases of State2 hmm features." % GC.GFF in msgs
    assert "Successfully extracted 1 features from within 0bp of State1 hmm annotations." in msgs
    out = _run(cli, tmp_path, "N2", ["--gffIn", GC.GFF, "--gffFeatures", "no_such_type", "--gffRange", "100000"])
    assert not any(f.startswith("featuresIn_") for f in os.listdir(out))


def test_cli_gffIn_without_gffFeatures_writes_nothing(fake_cli, tmp_path, caplog):  # noqa: F811
    cli, _made = fake_cli
    with caplog.at_level(logging.INFO, logger="frisk"):
        out = _run(cli, tmp_path, "G", ["--hmmKLD", "--gffIn", GC.GFF, "--gffRange", "1000"])
    assert not any(f.startswith("featuresIn_") for f in os.listdir(out)) and os.path.isfile(out / "a.gff3")
    assert any("--gffFeatures" in m and r.levelno == logging.INFO for m, r in zip(_messages(caplog), caplog.records))
    assert not any("not available" in m for m in _messages(caplog))
    # and --gffFeatures without --gffIn is no step at all
    out = _run(cli, tmp_path, "G2", ["--gffFeatures", "gene"])
    assert not any(f.startswith("featuresIn_") for f in os.listdir(out))


def test_cli_not_reached_under_exitAfter(fake_cli, tmp_path):  # noqa: F811
    cli, _made = fake_cli
    out = _run(cli, tmp_path, "E", ["--gffIn", GC.GFF, "--gffFeatures", "gene", "--exitAfter", "WindowKLD"])
    assert os.path.isfile(out / "raw_window_scores.bed") and not any(f.startswith("featuresIn_") for f in os.listdir(out))


def test_cli_missing_annotation_fails_before_the_scan(fake_cli, tmp_path, caplog):  # noqa: F811
    cli, _made = fake_cli
    out = tmp_path / "M"
    with pytest.raises(SystemExit) as err:
        cli.main(BASE + ["-t", str(out), "--gffIn", str(tmp_path / "nothing_here.gff3"), "--gffFeatures", "gene"])
    assert err.value.code == 1 and not os.path.exists(out)                                      # not even --tempDir was made
    assert any("nothing_here.gff3" in m for m in _messages(caplog))


def test_cli_negative_range_is_rejected(fake_cli, tmp_path, caplog):  # noqa: F811
    cli, _made = fake_cli
    out = tmp_path / "R"
    with pytest.raises(SystemExit) as err:
        cli.main(BASE + ["-t", str(out), "--gffIn", GC.GFF, "--gffFeatures", "gene", "--gffRange", "-1"])
    assert err.value.code == 1 and not os.path.exists(out)
    assert any("--gffRange" in m for m in _messages(caplog))
    assert cli.mainArgs(["-H", GC.FASTA]).gffRange == 0                                          # the default


def test_unavailable_no_longer_lists_gffIn():
    from frisk_amd.cli import build_parser, unavailable
    args = build_parser().parse_args(["-H", "h.fa", "--gffIn", "a.gff3", "--gffFeatures", "gene"])
    assert unavailable(args) == []
    args = build_parser().parse_args(["-H", "h.fa", "--gffIn", "a.gff3", "--cluster", "SPECTRAL", "--graphics", "g.pdf"])
    got = unavailable(args)
    assert [opt for opt, _why in got] == ["cluster", "graphics"] and got[-1][0] == "graphics"


def test_cli_every_other_output_is_byte_for_byte_the_same(fake_cli, tmp_path, capsys):  # noqa: F811
    cli, _made = fake_cli
    annotation = open(GC.GFF, "rb").read()
    plain = _run(cli, tmp_path, "P", ["--hmmKLD"])
    plain_out = capsys.readouterr().out
    with_gff = _run(cli, tmp_path, "W", ["--hmmKLD", "--gffIn", GC.GFF, "--gffFeatures", "gene", "mRNA", "--gffRange", "25"])
    assert capsys.readouterr().out == plain_out
    assert sorted(set(os.listdir(with_gff)) - set(os.listdir(plain))) == sorted([ANOM, STATE1, STATE2])
    assert set(os.listdir(plain)) <= set(os.listdir(with_gff))
    for f in ("raw_window_scores.bed", "a.gff3", "states.gff3", "RIP_annotation.gff3"):
        assert os.path.getsize(plain / f) > 0 and open(with_gff / f, "rb").read() == open(plain / f, "rb").read(), f
    assert open(GC.GFF, "rb").read() == annotation                                              # the annotation itself is untouched
