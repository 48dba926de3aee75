"""--spikeNormal end to end: the same job with and without the option.  The anomaly rows of the projection's input, the score
table, --gffOutfile and the RIP / HMM files do not change; the spiked rows are the windows postprocess.spike_rows names, with the
oracle's vectors, behind the anomaly rows; the cluster GFF3 keeps the anomaly rows and the spiked ones get a file of their own."""
import glob
import os
import pickle

import numpy as np
import pytest

from golden_util import GOLD

pytestmark = pytest.mark.gpu

FA = os.path.join(GOLD, "inputs", "markov_islands.fa")
BASE = ["-H", FA, "-m", "1", "-k", "4", "-w", "400", "-i", "150", "-F", "0.05", "--RIP", "--hmmKLD", "--runProjection", "PCA",
        "--cluster", "KMEANS", "--dumpPCAdata", "--gffOutfile", "a.gff3", "--pcaMin", "1", "--pcaMax", "4", "--seed", "1"]
CLUSTER_GFF = "PCA_KMEANS_k_2_cluster_labeled_windows_a.gff3"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from frisk_amd.cli import main
    plain, spike = tmp_path_factory.mktemp("plain"), tmp_path_factory.mktemp("spike")
    assert main(BASE + ["-t", str(plain)]) == 0
    assert main(BASE + ["-t", str(spike), "--spikeNormal"]) == 0
    return plain, spike


def load(path):
    with open(path, "rb") as fh:
        return pickle.load(fh)


def test_anomaly_rows_are_unchanged_and_spiked_rows_follow(runs):
    from frisk_amd import postprocess as pp
    from frisk_amd.cli import _load_window_cache
    from frisk_amd.fasta import readFasta
    from frisk_amd.projection import proportions_from_forward
    from oracle import frisk_oracle_np as N
    plain, spike = runs
    labels0, counts0 = load(plain / "anomLabels"), load(plain / "anomCounts")
    labels1, counts1, mask = load(spike / "anomLabels"), load(spike / "anomCounts"), load(spike / "anomSpike")
    n_anom = len(labels0)
    assert n_anom >= 2 and counts0.shape == (n_anom, 180)
    assert labels1[:n_anom].tolist() == labels0.tolist() and counts1[:n_anom].tobytes() == counts0.tobytes()
    # the spiked rows: spike_rows on the run's own score table (the window cache holds it at full precision)
    table = _load_window_cache(glob.glob(str(spike / "*_KLD_window_*.p"))[0], True)
    with np.errstate(divide="ignore"):
        logs = np.log10(np.where(table.kld_is_int0 != 0, 0.0, table.kld))
    rows = pp.spike_rows(logs, pp.pickedKLD(logs, float(np.log10(0.05))), n_anom)
    n_spike = len(rows)
    assert 0 < n_spike <= n_anom
    assert mask.dtype == bool and mask.tolist() == [False] * n_anom + [True] * n_spike
    assert len(labels1) == n_anom + n_spike == len(counts1)
    assert labels1[n_anom:, 0].tolist() == ["%s:%d:%d" % (table.names[table.seq_index[r]], table.start[r], table.stop[r]) for r in rows]
    assert not set(labels1[n_anom:, 0].tolist()) & set(labels0[:, 0].tolist())
    names, seqs = readFasta(FA)
    fasta = dict(zip(names, seqs))
    for lab, row in zip(labels1[:, 0].tolist(), counts1):
        nm, a, b = lab.rsplit(":", 2)
        seq = fasta[nm][int(a) - 1:int(b)]
        seq = seq if isinstance(seq, str) else seq.decode()
        assert row.tolist() == proportions_from_forward(N.forward_counts(N.Encoded(seq), 1, 4)[0], 1, 4).tolist(), lab


def test_other_outputs_are_byte_identical(runs):
    plain, spike = runs
    same = ["raw_window_scores.bed", "a.gff3", "RIP_annotation.gff3", "2StateHmm.gff3"]
    for f in same:
        if f == "RIP_annotation.gff3" and not os.path.exists(plain / f):
            assert not os.path.exists(spike / f)
            continue
        assert open(plain / f, "rb").read() == open(spike / f, "rb").read(), f
    extra = sorted(set(os.listdir(spike)) - set(os.listdir(plain)))
    assert extra == ["anomSpike", "spikeNormal_" + CLUSTER_GFF]


def test_cluster_gff_keeps_the_anomalies_and_the_spikes_get_their_own(runs):
    plain, spike = runs
    n_anom = len(load(plain / "anomLabels"))
    n_spike = int(load(spike / "anomSpike").sum())
    rows = lambda p: [ln.split("\t") for ln in open(p).read().splitlines()[1:]]        # noqa: E731
    old, new, extra = rows(plain / CLUSTER_GFF), rows(spike / CLUSTER_GFF), rows(spike / ("spikeNormal_" + CLUSTER_GFF))
    assert len(old) == len(new) == n_anom and len(extra) == n_spike
    for o, n in zip(old, new):                  # the same rows; the class is the joint clustering's
        assert o[:2] == n[:2] and o[3:] == n[3:] and n[2].startswith("Class_")
    labels = load(spike / "anomLabels")[:, 0].tolist()
    assert [":".join((r[0], r[3], r[4])) for r in new + extra] == labels
    assert open(spike / ("spikeNormal_" + CLUSTER_GFF)).readline() == "##gff-version 3\n"


def test_spike_normal_without_projection_only_warns(tmp_path, caplog):
    import logging
    from frisk_amd.cli import main
    with caplog.at_level(logging.WARNING, logger="frisk"):
        assert main(["-H", FA, "-m", "1", "-k", "4", "-w", "400", "-i", "150", "-F", "0.05", "--gffOutfile", "a.gff3", "--spikeNormal",
                     "-t", str(tmp_path)]) == 0
    assert any("--spikeNormal has no effect" in r.getMessage() for r in caplog.records)
    assert not [f for f in os.listdir(tmp_path) if "anom" in f or "spikeNormal" in f]
