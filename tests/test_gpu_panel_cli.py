"""python -m frisk_amd.regions --donors in a fresh child process on the device: markov_islands.fa with its hand-written
annotation as host and query, kat.fa and nheavy.fa as donors.  Every donor column against the windowKLD column of a separate
single-profile run of the module (-H donor -Q markov_islands.fa), as text; -O against the run without --donors, as bytes;
nearest / margin recomputed from the cells."""
import os
import subprocess
import sys

import pytest

from golden_util import INPUTS

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FA = os.path.join(INPUTS, "markov_islands.fa")
GFF = os.path.join(INPUTS, "markov_islands.gff3")
DONORS = [os.path.join(INPUTS, "kat.fa"), os.path.join(INPUTS, "nheavy.fa")]


def _start(argv, tmp_path):
    env = dict(os.environ, FRISK_FLOAT_REPR="py3", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.Popen([sys.executable, "-m", "frisk_amd.regions"] + argv, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)


def _finish(proc):
    _out, err = proc.communicate(timeout=300)
    assert proc.returncode == 0, err


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    return head, [dict(zip(head, l.split("\t"))) for l in lines[1:-1]]


def test_regions_module_scores_the_annotation_against_donors(tmp_path):
    gff = tmp_path / "on_the_fasta.gff3"                # the annotation without the record on chrM, which the FASTA does not hold
    gff.write_text("".join(l for l in open(GFF) if not l.startswith("chrM")))
    common = ["--gff", str(gff), "--RIP"]
    _finish(_start(["-H", FA, "-t", "out", "--donors"] + DONORS + common, tmp_path))
    # the runs to compare with, side by side, each in a directory of its own (no cache to share): without --donors, and
    # -H donor -Q markov_islands.fa per donor
    others = [_start(["-H", FA, "-t", "plain"] + common, tmp_path)]
    others += [_start(["-H", d, "-Q", FA, "-t", "single_" + os.path.basename(d)] + common, tmp_path) for d in DONORS]
    for proc in others:
        _finish(proc)
    labels = ["markov_islands.fa", "kat.fa", "nheavy.fa"]
    head, rows = _table(tmp_path / "out" / "region_donor_scores.tsv")
    assert head == ["name", "start", "stop", "length", "id"] + labels + ["nearest", "margin"] and len(rows) == 21
    for label in labels:                                # the genome k-mer caches of the main command line, one per genome
        assert (tmp_path / "out" / ("%s_kmers_1_8_genome.p" % label)).is_file(), label
    # -O: the run without --donors
    assert (tmp_path / "out" / "region_scores.tsv").read_bytes() == (tmp_path / "plain" / "region_scores.tsv").read_bytes()
    assert not (tmp_path / "plain" / "region_donor_scores.tsv").exists()
    _, host = _table(tmp_path / "plain" / "region_scores.tsv")
    assert [r["markov_islands.fa"] for r in rows] == [r["windowKLD"] for r in host]
    for c in ("name", "start", "stop", "length", "id"):
        assert [r[c] for r in rows] == [r[c] for r in host], c
    # every donor column: a separate single-profile run, its profile computed afresh
    for donor, label in zip(DONORS, labels[1:]):
        _, single = _table(tmp_path / ("single_" + label) / "region_scores.tsv")
        assert [r[label] for r in rows] == [r["windowKLD"] for r in single], label
    # nearest / margin from the cells (FRISK_FLOAT_REPR=py3: a cell is repr(float), so float(cell) is the value itself)
    # (the donors are tiny genomes: at K = 8 most regions hold a max-mer that a donor lacks - nan, the reference's
    # ZeroDivisionError - so rows with two finite cells may be few here; test_panel_cpu.py has them by construction)
    for r in rows:
        vals = sorted((float(r[l]), i) for i, l in enumerate(labels) if r[l] != "nan")
        if not vals:
            assert (r["nearest"], r["margin"]) == (".", "."), r
            continue
        assert r["nearest"] == labels[vals[0][1]], r
        if len(vals) < 2:
            assert r["margin"] == ".", r
        else:
            assert float(r["margin"]) == vals[1][0] - vals[0][0], r
    assert sum(r["markov_islands.fa"] != "nan" for r in rows) >= 15
