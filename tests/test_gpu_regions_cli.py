"""python -m frisk_amd.regions in a fresh child process on the device: markov_islands.fa with its hand-written annotation, every
row of the table against the reference's scan-loop iteration on the region's slice (tests/ranges_cases.py: status, GC and RIP
indices exactly, KLD within kld_oracle_hp.bound(scale))."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kld_oracle_hp as H
import ranges_cases as R
from golden_util import INPUTS
from oracle import frisk_oracle as O
from oracle import frisk_oracle_np as N

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FA = os.path.join(INPUTS, "markov_islands.fa")
GFF = os.path.join(INPUTS, "markov_islands.gff3")


def _run(argv, tmp_path):
    env = dict(os.environ, FRISK_FLOAT_REPR="py3", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "frisk_amd.regions"] + argv, cwd=str(tmp_path), env=env, capture_output=True,
                          text=True, timeout=300)


def test_regions_module_scores_the_annotation(tmp_path):
    from frisk_amd import regions
    from frisk_amd.engine import ScanResult
    gff = tmp_path / "on_the_fasta.gff3"                # the annotation without the record on chrM, which the FASTA does not hold
    gff.write_text("".join(l for l in open(GFF) if not l.startswith("chrM")))
    p = _run(["-H", FA, "-t", "out", "--gff", str(gff), "--RIP"], tmp_path)
    assert p.returncode == 0, p.stderr
    lines = (tmp_path / "out" / "region_scores.tsv").read_text().split("\n")
    assert lines[0].split("\t") == ["name", "start", "stop", "length", "windowKLD", "GC", "PI", "SI", "CRI", "id", "note"]
    recs = regions.read_gff_regions(str(gff))
    assert len(recs) == 21 and len(lines) == len(recs) + 2 and lines[-1] == ""
    names = [n for n, _ in O.iter_fasta(FA)]
    seqs = H.read_fasta(FA)
    prof = H.profile(seqs, 1, 8)
    rows = [(names.index(n), a, b) for n, a, b, _ in recs]
    exp = R.expect_rows(seqs, prof, N.genome_ivom_table(prof[0], prof[1], 1, 8), rows, 1, 8)
    got = [l.split("\t") for l in lines[1:-1]]
    notes = {".": R.KEPT, "unresolved": 0, "ZeroDivisionError": R.KEPT | R.ZERO_WEIGHT, "noMaxmer": R.KEPT | R.NO_MAXMER}
    for g, (n, a, b, ident) in zip(got, recs):
        assert g[:4] == [n, str(a + 1), str(b), str(b - a)] and g[9] == ident, g
    res = ScanResult(status=np.array([notes[g[10]] for g in got], np.uint32), nn=np.array([e["nn"] for e in exp], np.int64),
                     kld=np.array([float(g[4]) for g in got]), gc=np.array([float(g[5]) for g in got]),
                     pi=np.array([float(g[6]) for g in got]), si=np.array([float(g[7]) for g in got]),
                     cri=np.array([float(g[8]) for g in got]))
    R.check("regions module, markov_islands.gff3", res, exp)
    assert sum(e["flag"] == H.OK for e in exp) >= 15
    assert (tmp_path / "out" / "markov_islands.fa_kmers_1_8_genome.p").is_file()


def test_regions_module_names_the_record_it_cannot_place(tmp_path):
    p = _run(["-H", FA, "-t", "out", "--gff", GFF, "--gffFeatures", "gene"], tmp_path)
    assert p.returncode == 1
    assert "chrM:10-800" in p.stderr and not (tmp_path / "out" / "region_scores.tsv").exists()
