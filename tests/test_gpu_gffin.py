"""--gffIn end to end on the GPU: one `python -m frisk_amd` run with -F, --hmmKLD, --gffIn, --gffFeatures and --gffRange; the three
featuresIn_* files against the brute-force statement of `bedtools window -w W -u` on the run's own anomaly and HMM GFF3."""
import os
import subprocess
import sys

import pytest

import gffin_cases as GC

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TYPES = ["gene", "tRNA"]
RANGE = 10


def test_cli_gffIn_end_to_end(tmp_path):
    out = tmp_path / "G"
    assert GC.FASTA.startswith(REPO) and GC.GFF.startswith(REPO)                 # nothing is read from outside the repository
    cmd = [sys.executable, "-m", "frisk_amd", "-H", GC.FASTA, "-m", "2", "-k", "4", "-w", "400", "-i", "150", "-t", str(out),
           "-F", "0.08", "--hmmKLD", "--hmmOutfile", "states.gff3", "--gffOutfile", "a.gff3",
           "--gffIn", GC.GFF, "--gffFeatures"] + TYPES + ["--gffRange", str(RANGE)]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "not available" not in p.stderr and "gffIn features" in p.stderr         # no warning; the lap is in the timing line
    base = os.path.basename(GC.GFF)
    all_rows = [line for line, f in GC.gff_rows(GC.GFF) if f[2] in TYPES]
    anomalies = [(f[0], int(f[3]), int(f[4])) for _line, f in GC.gff_rows(out / "a.gff3")]   # BED: the table's numbers as they are
    states = GC.gff_rows(out / "states.gff3")
    assert len(anomalies) > 1 and {f[2] for _line, f in states} == {"State1", "State2"}
    for name, regions, what in (("featuresIn_thresholded_Anomalies_" + base, anomalies, "anomaly"),
                                ("featuresIn_hmm_State1_" + base, GC.gff_as_bed(states, ["State1"]), "State1 hmm"),
                                ("featuresIn_hmm_State2_" + base, GC.gff_as_bed(states, ["State2"]), "State2 hmm")):
        want = GC.expected_lines(TYPES, regions, RANGE)
        got = open(out / name, newline="").read()
        print("%s: %d of %d records kept" % (name, len(want), len(all_rows)))
        assert got == "".join(want), name
        assert 0 < len(want) < len(all_rows), name                                   # some kept, some not
        assert "Successfully extracted %d features from within %dbp of %s annotations." % (len(want), RANGE, what) in p.stderr
    assert sorted(f for f in os.listdir(out) if f.startswith("featuresIn_")) == sorted(
        pre + base for pre in ("featuresIn_thresholded_Anomalies_", "featuresIn_hmm_State1_", "featuresIn_hmm_State2_"))
