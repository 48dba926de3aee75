"""No-GPU checks of --spikeNormal: postprocess.spike_rows (the definition of "the centre of the self population") on hand-written
tracks, projection.windowVectors' rules against a stub engine whose (X, nn, status) come from the numpy oracle, and the CLI's
row order, labels and mask with that stub in place of the device."""
import argparse
import logging

import numpy as np
import pytest

from frisk_amd import _ffi
from frisk_amd import postprocess as pp
from frisk_amd.projection import feature_keys, mirror_keep, proportions_from_forward, revcomp_index
from frisk_amd.table import ScoreTable
from oracle import frisk_oracle_np as N

INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------ spike_rows
def test_spike_rows_takes_the_unpicked_rows_nearest_the_median():
    logs = np.array([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0])        # median 0
    picked = pp.pickedKLD(logs, 2.0)
    assert picked.tolist() == [False] * 5 + [True, True]
    assert pp.spike_rows(logs, picked, 1).tolist() == [3]
    assert pp.spike_rows(logs, picked, 3).tolist() == [2, 3, 4]
    assert pp.spike_rows(logs, picked, 2).tolist() == [2, 3]           # rows 2 and 4 tie at distance 1: table order
    assert pp.spike_rows(logs, picked, 4).tolist() == [1, 2, 3, 4]     # rows 1 and 5 tie at distance 2, but 5 is picked


def test_spike_rows_ties_break_by_table_order_and_come_back_in_table_order():
    logs = np.array([1.0, -1.0, 1.0, -1.0, 0.0, 5.0])                 # finite median = 0.5: distances .5 1.5 .5 1.5 .5 4.5
    picked = np.array([False, False, False, False, False, True])
    assert pp.spike_rows(logs, picked, 2).tolist() == [0, 2]           # three rows at 0.5: the first two of the table
    assert pp.spike_rows(logs, picked, 3).tolist() == [0, 2, 4]
    assert pp.spike_rows(logs, picked, 4).tolist() == [0, 1, 2, 4]     # rows 1 and 3 tie at 1.5


def test_spike_rows_leaves_out_unscored_rows_and_uses_them_nowhere():
    logs = np.array([-INF, 0.1, NAN, 0.0, -0.1, NAN, 4.0, -INF])       # finite: .1 0 -.1 4 -> median 0.05
    picked = pp.pickedKLD(logs, 3.0)
    assert picked.tolist() == [False, False, False, False, False, False, True, False]
    assert pp.spike_rows(logs, picked, 10).tolist() == [1, 3, 4]       # n above the candidates: all of them, never -inf / NaN
    assert pp.spike_rows(logs, picked, 1).tolist() == [1]              # |.1 - .05| = |0 - .05|: table order
    assert pp.spike_rows(logs, picked, 0).tolist() == []
    assert pp.spike_rows(logs, picked, 0).dtype == np.int64


def test_spike_rows_under_find_self_and_without_candidates():
    logs = np.array([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0])
    picked = pp.pickedKLD(logs, -2.0, find_self=True)                  # --findSelf picks the rows BELOW the cut
    assert picked.tolist() == [True, True] + [False] * 5
    assert pp.spike_rows(logs, picked, 3).tolist() == [2, 3, 4]
    assert pp.spike_rows(logs, picked, 5).tolist() == [2, 3, 4, 5, 6]
    assert pp.spike_rows(logs, np.ones(7, bool), 3).tolist() == []     # everything picked
    assert pp.spike_rows(np.array([NAN, -INF]), np.zeros(2, bool), 3).tolist() == []
    assert pp.spike_rows(np.zeros(0), np.zeros(0, bool), 3).tolist() == []


@pytest.mark.parametrize("find_self", [False, True])
def test_picked_mask_is_threshold_kld_s_selection(find_self):
    rows = [("a", 1, 10, 0.5, 0.4), ("a", 6, 15, 0, 0.4), ("a", 11, 20, NAN, 0.4), ("b", 1, 10, 3.0, 0.4), ("b", 6, 15, 0.01, 0.4),
            ("b", 11, 20, 1.0, 0.4)]
    table = ScoreTable.from_rows(rows)
    args = argparse.Namespace(findSelf=find_self, mergeDist=0)
    kld = np.where(table.kld_is_int0 != 0, 0.0, table.kld)
    with np.errstate(divide="ignore"):
        logs = np.log10(kld.reshape(-1, 1))
    _feats, chosen = pp.thresholdKLD(table, 0.0, args, merge=False)
    mask = pp.pickedKLD(logs, 0.0, find_self)
    assert sorted(table.rows(np.nonzero(mask)[0]), key=lambda r: r[:3]) == list(chosen)
    assert not mask[2]                                                  # a NaN row is never picked, under either rule


# ------------------------------------------------------------------------------------------------ windowVectors on a stub engine
class StubEngine:
    """Engine.window_vectors / read_seq / load_fasta from the numpy oracle: what the device must return."""
    device = 0

    def __init__(self, seqs=None, names=None):
        self.seqs, self.names = list(seqs or []), list(names or [])
        self.seq_lens = [len(s) for s in self.seqs]
        self.calls = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def load_fasta(self, path):
        from frisk_amd.fasta import readFasta
        self.names, self.seqs = readFasta(path)
        self.seqs = [s if isinstance(s, str) else s.decode() for s in self.seqs]
        self.seq_lens = [len(s) for s in self.seqs]
        return list(self.names)

    def read_seq(self, index, offset=0, n=None):
        return self.seqs[index][offset:offset + n].encode()

    def window_vectors(self, seq_index, start, stop, kmin, kmax, batch_rows=0):
        self.calls.append((list(map(int, seq_index)), list(map(int, start)), list(map(int, stop)), kmin, kmax))
        n = len(seq_index)
        X = np.full((n, len(feature_keys(kmin, kmax))), NAN)
        nn, status = np.zeros(n, np.int64), np.zeros(n, np.uint32)
        for r in range(n):
            enc = N.Encoded(self.seqs[int(seq_index[r])][int(start[r]):int(stop[r])])
            fwd = N.forward_counts(enc, kmin, kmax)[0]
            nn[r] = enc.n - int(enc.upper.sum())
            col = 0
            for x in range(kmin, kmax + 1):
                f = fwd[N.table_offset(kmin, x):N.table_offset(kmin, x + 1)]
                kept = (f + f[revcomp_index(x)])[mirror_keep(x)]
                if kept.sum() == 0:
                    status[r] |= _ffi.KVEC_EMPTY_ORDER | (1 << (_ffi.KVEC_ORDER_SHIFT + x))     # entries unspecified: left NaN
                else:
                    X[r, col:col + kept.size] = proportions_from_forward(f, x, x)
                col += kept.size
        return X, nn, status


RNG = np.random.default_rng(11)
SEQ = "".join(RNG.choice(list("ACGT"), size=600)) + "N" * 60 + "".join(RNG.choice(list("acgt"), size=100)) + "ACGTTGCA" * 20


def test_window_vectors_returns_the_oracle_rows():
    from frisk_amd.projection import windowVectors
    e = StubEngine([SEQ, SEQ[::-1]])
    X = windowVectors(e, [0, 1, 0], [0, 330, 300], [400, 800, 700], 1, 4)      # the last: 60 N + 40 lowercase of 400
    for row, (s, a, b) in zip(X, [(0, 0, 400), (1, 330, 800), (0, 300, 700)]):
        fwd = N.forward_counts(N.Encoded(e.seqs[s][a:b]), 1, 4)[0]
        assert row.tolist() == proportions_from_forward(fwd, 1, 4).tolist()
    assert windowVectors(e, [], [], [], 1, 6).shape == (0, 2772)


def test_window_vectors_applies_the_thirty_percent_rule_with_symmetric_counts_text():
    from frisk_amd.projection import windowVectors
    e = StubEngine([SEQ])
    # 140 bases, 42 of them N: exactly 30 % -> dropped (>=); 41 of 140 -> kept
    with pytest.raises(ValueError) as err:
        windowVectors(e, [0], [502], [642], 1, 3, labels=["chrA:503:642"])
    assert str(err.value) == "sequence 'chrA:503:642' has >= 30 % unresolved bases: no k-mer vector"
    assert windowVectors(e, [0], [501], [641], 1, 3).shape == (1, 44)
    with pytest.raises(ValueError, match="30 % unresolved"):           # lowercase is unresolved for the rule, counted for the vector
        windowVectors(e, [0], [660], [760], 1, 3)


def test_window_vectors_names_the_row_and_the_empty_order():
    from frisk_amd.projection import windowVectors
    e = StubEngine([SEQ])
    with pytest.raises(ValueError) as err:
        windowVectors(e, [0, 0], [0, 100], [50, 103], 1, 4)
    assert "row 1 " in str(err.value) and "order 4" in str(err.value) and "0:101:103" in str(err.value)


def test_window_vectors_orders_above_the_kernel_take_the_old_route(monkeypatch, caplog):
    import frisk_amd.projection as P
    e = StubEngine([SEQ])
    seen = []

    def fake_symmetric(labelled, pcaMin, pcaMax, device=0):
        seen.append((labelled, pcaMin, pcaMax, device))
        return np.array([[lab] for lab, _ in labelled]), np.arange(len(labelled) * 3.0).reshape(len(labelled), 3)
    monkeypatch.setattr(P, "symmetricCounts", fake_symmetric)
    monkeypatch.setattr(P, "_fallback_logged", False)
    with caplog.at_level(logging.INFO, logger="frisk_amd"):
        X = P.windowVectors(e, [0, 0], [5, 700], [25, 720], 1, 8)
        P.windowVectors(e, [0], [5], [25], 2, 9)
    assert X.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    assert seen[0] == ([("0:6:25", SEQ[5:25]), ("0:701:720", SEQ[700:720])], 1, 8, 0)
    assert e.calls == []                                                # the kernel was not called
    assert len([r for r in caplog.records if "count dump" in r.getMessage()]) == 1      # logged once


# ------------------------------------------------------------------------------------------------ the CLI's rows, stub for the device
def _spiked(monkeypatch, tmp_path, klds, threshold, find_self=False, names=("s0", "s1")):
    import frisk_amd.cli as cli
    import frisk_amd.engine as engine_mod
    fa = tmp_path / "q.fa"
    seqs = ["".join(np.random.default_rng(i).choice(list("ACGT"), size=400)) for i in range(len(names))]
    fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    rows = []
    for i, k in enumerate(klds):                                        # windows of 100 bases, step 50, five per scaffold
        rows.append((names[i // 5], 50 * (i % 5) + 1, 50 * (i % 5) + 100, k, 0.5))
    table = ScoreTable.from_rows(rows)
    stub = StubEngine()
    monkeypatch.setattr(engine_mod, "Engine", lambda *a, **k: stub)
    args = cli.build_parser().parse_args(["-H", str(fa), "--runProjection", "PCA", "--spikeNormal", "--pcaMin", "1", "--pcaMax", "3"]
                                         + (["--findSelf"] if find_self else []))
    kld = np.where(table.kld_is_int0 != 0, 0.0, table.kld)
    with np.errstate(divide="ignore"):
        logKLD = np.log10(kld.reshape(-1, 1))
    feats, _ = pp.thresholdKLD(table, threshold, args, merge=False)
    out = cli._spiked_counts(args, table, logKLD, threshold, feats, str(fa), 0, cli._Clock())
    return out, stub, seqs, feats


def test_cli_rows_anomalies_first_then_spiked_windows_in_one_call(monkeypatch, tmp_path):
    klds = [1.0, 1.3, 100.0, 0.9, 1.0, 1.2, 50.0, 0.5, 1.0, 1.0]       # log10 median = 0.0 (1.0); rows 2 and 6 anomalous
    (labelled, labels, counts, spiked), stub, seqs, feats = _spiked(monkeypatch, tmp_path, klds, 1.5)
    assert labelled == ["s0:101:200", "s1:51:150"] == [":".join(map(str, f[:3])) for f in feats]
    assert labels[:, 0].tolist() == labelled + ["s0:1:100", "s0:201:300"]           # rows 0 and 4: log10 = 0 exactly, table order
    assert spiked.tolist() == [False, False, True, True]
    assert len(stub.calls) == 1 and stub.calls[0] == ([0, 1, 0, 0], [100, 50, 0, 200], [200, 150, 100, 300], 1, 3)
    for row, (s, a, b) in zip(counts, [(0, 100, 200), (1, 50, 150), (0, 0, 100), (0, 200, 300)]):
        assert row.tolist() == proportions_from_forward(N.forward_counts(N.Encoded(seqs[s][a:b]), 1, 3)[0], 1, 3).tolist()


def test_cli_rows_without_anomalies_or_without_candidates(monkeypatch, tmp_path, caplog):
    with caplog.at_level(logging.INFO, logger="frisk"):
        (labelled, labels, counts, spiked), stub, _s, _f = _spiked(monkeypatch, tmp_path, [1.0] * 10, 1.5)
    assert labelled == [] and labels.shape == (0, 1) and counts.shape == (0, 44) and spiked is None and stub.calls == []
    assert any("no anomalous window" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="frisk"):                # everything is picked: nothing ordinary is left
        (labelled, labels, counts, spiked), stub, _s, _f = _spiked(monkeypatch, tmp_path, [10.0] * 10, 0.5)
    assert len(labelled) == 10 and labels[:, 0].tolist() == labelled and counts.shape == (10, 44) and spiked is None
    assert any("no ordinary window" in r.getMessage() for r in caplog.records)


def test_cli_find_self_spikes_from_the_other_side(monkeypatch, tmp_path):
    klds = [0.001, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 0.002, 1.0, 4.0]      # --findSelf: rows 0 and 7 (below the cut) are the set
    (labelled, labels, _c, spiked), _stub, _s, _f = _spiked(monkeypatch, tmp_path, klds, -2.0, find_self=True)
    assert labelled == ["s0:1:100", "s1:101:200"]
    assert labels[2:, 0].tolist() == ["s0:51:150", "s0:101:200"] and spiked.tolist() == [False, False, True, True]
