"""python -m frisk_amd.regions --refine in fresh child processes on the device: markov_islands.fa with its hand-written annotation,
the table against the numpy restatement of frisk_amd/refine.py, -O unchanged, and the newKLD column against a plain run on the
refined BED, byte for byte."""
import os
import subprocess
import sys

import pytest

import kld_oracle_hp as H
from golden_util import INPUTS
from oracle import frisk_oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FA = os.path.join(INPUTS, "markov_islands.fa")
GFF = os.path.join(INPUTS, "markov_islands.gff3")


def _run(argv, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("FRISK_FLOAT_REPR", None)
    return subprocess.run([sys.executable, "-m", "frisk_amd.regions"] + argv, cwd=str(cwd), env=env, capture_output=True, text=True,
                          timeout=300)


def test_refine_table_equals_the_restatement_and_its_bed_scores_the_same(tmp_path):
    from frisk_amd import postprocess as pp, refine, regions
    gff = tmp_path / "on_the_fasta.gff3"                # the annotation without the record on chrM, which the FASTA does not hold
    gff.write_text("".join(l for l in open(GFF) if not l.startswith("chrM")))
    p = _run(["-H", FA, "-t", "plain", "--gff", str(gff)], tmp_path)
    assert p.returncode == 0, p.stderr
    p = _run(["-H", FA, "-t", "ref", "--gff", str(gff), "--refine", "300"], tmp_path)
    assert p.returncode == 0, p.stderr
    plain = (tmp_path / "plain" / "region_scores.tsv").read_bytes()
    assert (tmp_path / "ref" / "region_scores.tsv").read_bytes() == plain
    recs = regions.read_gff_regions(str(gff))
    names = [n for n, _ in O.iter_fasta(FA)]
    seqs = H.read_fasta(FA)
    sym, _ = H.profile(seqs, 1, 8)
    want = refine.refine_rows(seqs, sym, 1, [(names.index(n), a, b) for n, a, b, _ in recs], 300, refine.default_order(1, 8), kmax=8)
    lines = (tmp_path / "ref" / "region_refined.tsv").read_text().split("\n")
    assert lines[0].split("\t") == regions.REFINE_COLUMNS and lines[-1] == "" and len(lines) == len(recs) + 2
    scores = [l.split("\t") for l in plain.decode().split("\n")[1:-1]]
    notes = []
    for i, ((name, a, b, ident), line) in enumerate(zip(recs, lines[1:-1])):
        f = line.split("\t")
        ns, ne = int(want.new_start[i]), int(want.new_stop[i])
        assert f[:5] == [name, str(a + 1), str(b), str(b - a), ident], f
        assert f[5:10] == [str(ns + 1), str(ne), str(ne - ns), str(ns - a), str(ne - b)], f
        assert f[10:12] == [pp.py2_str(int(want.gain_start[i]) / 2.0 ** 32), pp.py2_str(int(want.gain_stop[i]) / 2.0 ** 32)], f
        assert f[12] == str(int(want.flank_used[i])) and f[13] == scores[i][4], f
        assert f[15] == ("short" if int(want.flank_used[i]) == 0 else "." if int(want.status[i]) & 1 else "unresolved"), f
        notes.append(f[15])
    assert notes.count(".") >= 15 and sum(int(f) != 0 for l in lines[1:-1] for f in l.split("\t")[8:10]) >= 20
    # the refined BED through --bed: its windowKLD column is the table's newKLD column
    bed = tmp_path / "ref" / "regions_refined.bed"
    assert bed.read_text() == "".join("%s\t%d\t%d\t%s\n" % (n, int(want.new_start[i]), int(want.new_stop[i]), ident)
                                      for i, (n, _, _, ident) in enumerate(recs))
    p = _run(["-H", FA, "-t", "again", "--bed", str(bed)], tmp_path)
    assert p.returncode == 0, p.stderr
    again = (tmp_path / "again" / "region_scores.tsv").read_text().split("\n")[1:-1]
    assert [l.split("\t")[14] for l in lines[1:-1]] == [l.split("\t")[4] for l in again]
    assert [l.split("\t")[-2] for l in again] == [ident for _, _, _, ident in recs]
