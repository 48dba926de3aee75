"""--updateHMM without a GPU: the reference's updateHMM on its recorded cases, the three rules the CLI adds around it, the new ABI
symbols, the qualification of the device-HMM test inputs (tests/golden/hmm_gpu.json), and the CLI on an oracle-backed engine."""
import json
import logging
import os
import re

import numpy as np
import pytest

import hmm_gpu_cases as H
from frisk_amd import postprocess as pp
from frisk_amd.hmm import GaussianHMM2

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden")
UPDATE = json.load(open(os.path.join(GOLD, "update_hmm.json")))
HMM = json.load(open(os.path.join(GOLD, "hmm_gpu.json")))


# ------------------------------------------------------------------------------------------------- the reference's function
def test_recorded_cases_cover_what_the_issue_names():
    names = {c["name"] for c in UPDATE["cases"]}
    assert {"ties_at_equal_distance", "boundary_on_an_anomaly_edge", "several_scaffolds",
            "string_sorted_order_and_single_windows"} <= names
    tie = next(c for c in UPDATE["cases"] if c["name"] == "ties_at_equal_distance")
    assert tie["expected"][0] == ["s1", "901", "1000"]          # 1200 is 200 from 1000 and from 1400: the first in list order
    assert tie["expected"][1] == ["s1", "501", "1400"]          # 1700 is 300 from 1400 and from 2000
    many = next(c for c in UPDATE["cases"] if c["name"] == "string_sorted_order_and_single_windows")
    starts = [int(f[1]) for f in many["fine"] if f[0] == "chr2"]
    assert starts != sorted(starts) and any(int(f[2]) - int(f[1]) == 999 for f in many["fine"])
    assert len({f[0] for f in next(c for c in UPDATE["cases"] if c["name"] == "several_scaffolds")["fine"]}) == 3


@pytest.mark.parametrize("case", UPDATE["cases"], ids=lambda c: c["name"])
def test_updateHMM_reproduces_the_reference(case):
    fine = [tuple(r) for r in case["fine"]]
    anomalies = [tuple(r) for r in case["anomalies"]]
    assert [list(r) for r in pp.updateHMM(fine, anomalies)] == case["expected"]
    # integer fields give the same answer (the CLI's records carry ints), and a generator of intervals is consumed once
    ints = [(a[0], int(a[1]), int(a[2])) + a[3:] for a in anomalies]
    assert [list(r) for r in pp.updateHMM(iter(fine), ints)] == case["expected"]


def test_updateHMM_raises_keyerror_like_the_reference():
    assert UPDATE["missing_scaffold_raises"].startswith("KeyError")
    with pytest.raises(KeyError):
        pp.updateHMM([("s1", "1", "100", "State1")], [("s2", "1", "50")])


# ----------------------------------------------------------------------------------------------------- the CLI's three rules
def test_refine_keeps_what_cannot_be_snapped_and_carries_fields(caplog):
    fine = [("s1", "1", "1000", "State1"), ("s1", "501", "3000", "State2")]
    anomalies = [("s1", 400, 2900, "0.5", "0.1", "0.3"),        # snapped: 501 .. 3000
                 ("s9", 10, 20, "0.4"),                          # no fine interval on the scaffold: kept
                 ("s1", 900, 1100, "0.3"),                       # both ends snap to 1000: left >= right, kept
                 ("s1", 2950, 420, "0.2")]                       # snapped left 3000 > right 501: kept
    with caplog.at_level(logging.INFO, logger="frisk"):
        got, kept = pp.refineAnomalies(fine, anomalies)
    assert got == [("s1", 501, 3000, "0.5", "0.1", "0.3"), anomalies[1], anomalies[2], anomalies[3]] and kept == 3
    lines = [r.getMessage() for r in caplog.records if r.levelno == logging.INFO]
    assert sum("keeps its boundaries" in ln for ln in lines) == 3
    assert sum("no fine HMM interval" in ln for ln in lines) == 1
    assert [ln for ln in lines if ln.startswith("Refined")] == ["Refined 1 of 4 anomalies to fine HMM boundaries; 3 kept as they were."]
    # string fields stay strings
    assert pp.refineAnomalies(fine, [("s1", "400", "2900", "0.5")], emit=lambda s: None)[0] == [("s1", "501", "3000", "0.5")]


@pytest.mark.parametrize("case", UPDATE["cases"], ids=lambda c: c["name"])
def test_refine_equals_updateHMM_where_the_rules_do_not_apply(case):
    fine = [tuple(r) for r in case["fine"]]
    anomalies = [tuple(r) for r in case["anomalies"]]
    got, kept = pp.refineAnomalies(fine, anomalies, emit=lambda s: None)
    n_kept = 0
    for a, g, e in zip(anomalies, got, case["expected"]):
        if int(e[1]) >= int(e[2]):
            assert g == a
            n_kept += 1
        else:
            assert list(g[:3]) == e and g[3:] == a[3:]
    assert kept == n_kept < len(anomalies)


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_device_hmm_symbols_are_declared_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    from frisk_amd import _ffi
    text = open(os.path.join(REPO, "include", "frisk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    table = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    for name in ("frisk_hmm_fit_gpu", "frisk_hmm_viterbi_gpu"):
        assert re.search(r"\bint\s+%s\s*\(\s*int\s+device\b" % name, text), name
        assert name in table and getattr(_ffi.lib(), name) is not None
    # the host entry points with the device in front
    host = {n: a for n, _r, a in _ffi.SYMBOLS}
    import ctypes as C
    assert table["frisk_hmm_fit_gpu"][1] == [C.c_int] + host["frisk_hmm_fit"]
    assert table["frisk_hmm_viterbi_gpu"][1] == [C.c_int] + host["frisk_hmm_viterbi"]
    # argument checks come before any device is touched
    lib = _ffi.lib()
    x = np.array([0.1, float("nan")])
    out = np.zeros(2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert lib.frisk_hmm_fit_gpu(0, p(x), 2, 10, 1e-2, 1e-3, 1e-2, p(out), p(out), p(out), p(np.zeros(4)), None, None) == _ffi.E_ARG
    off = np.array([0, 2, 1], dtype=np.int64)
    assert lib.frisk_hmm_viterbi_gpu(0, p(x), p(off), 2, p(out), p(out), p(out), p(np.zeros(4)), p(np.zeros(2, np.int8))) == _ffi.E_ARG
    # a non-finite score inside the decoded range, as the header says - also before any device is touched; outside it, it is not read
    fine = np.array([0, 1, 2], dtype=np.int64)
    states = np.zeros(2, np.int8)
    good = (p(np.array([0.04, 0.13])), p(np.array([2e-4, 1.5e-3])), p(np.array([0.6, 0.4])), p(np.array([0.97, 0.03, 0.08, 0.92])))
    for v in (float("nan"), float("inf"), -float("inf")):
        assert lib.frisk_hmm_viterbi_gpu(0, p(np.array([0.1, v])), p(fine), 2, *good, p(states)) == _ffi.E_ARG
        assert lib.frisk_hmm_viterbi_gpu(0, p(np.array([v, 0.1])), p(fine[1:]), 1, *good, p(states)) != _ffi.E_ARG
    with pytest.raises(ValueError):
        GaussianHMM2(native="cuda")


# ----------------------------------------------------------------------------- the inputs of the device tests, qualified here
def test_golden_tolerance_is_the_stated_multiple_of_the_cpu_spread():
    assert HMM["factor"] == H.FACTOR == 8 and HMM["margin"] == H.MARGIN == 1e-9 and HMM["gap"] == H.GAP == 1e-6
    assert HMM["spread_numpy_host"] == max(c["spread_numpy_host"] for c in HMM["fit"].values())
    assert HMM["tolerance"] == 8 * HMM["spread_numpy_host"]
    assert set(HMM["fit"]) == set(H.FIT_CASES) and set(HMM["viterbi"]) == set(H.VITERBI_CASES)
    assert HMM["fit"]["rows_3m"]["n"] == 3000000 and HMM["fit"]["at_pieces"]["n"] == H.PIECES
    assert HMM["viterbi"]["long_segment"]["n"] == 600000 and HMM["viterbi"]["long_segment"]["segments"] == 1


@pytest.mark.parametrize("name", list(H.FIT_CASES))
def test_fit_inputs_regenerate_and_stay_clear_of_tol(name):
    """Same bytes as when the golden was made; the numpy specification (recomputed here except on the 3 M rows, where its
    recorded fit stands) and the host-native fit differ by no more than the recorded spread; and no round's log-likelihood
    gain is within 1e-6 of tol, so that an equal round count may be demanded of the device."""
    g = HMM["fit"][name]
    x = H.fit_input(name)
    assert x.size == g["n"] and H.sha(x) == g["sha256"]
    host = GaussianHMM2(native=True).fit(x)
    assert host.n_iter_ == g["numpy"]["n_iter_"]
    if name in H.BIG:
        spec_p, spec_ll, spec_lls = g["numpy"], g["numpy"]["loglik_"], g["numpy_lls"]
    else:
        spec = H.RecordingHMM().fit(x)
        spec_p, spec_ll, spec_lls = H.params(spec), spec.loglik_, spec.lls
        assert spec.n_iter_ == g["numpy"]["n_iter_"]
    sp = H.spread(spec_p, H.params(host), spec_ll, host.loglik_)
    print("%s: numpy against host-native spread %.3g (recorded %.3g)" % (name, sp, g["spread_numpy_host"]))
    assert sp <= HMM["spread_numpy_host"]
    gap = min(H.gap_from_tol(spec_lls), H.gap_from_tol(H.native_lls(x, host.n_iter_)))
    print("%s: smallest |gain - tol| = %.3g" % (name, gap))
    assert gap >= H.GAP


@pytest.mark.parametrize("name", [n for n in H.VITERBI_CASES if n != "long_segment"])
def test_viterbi_inputs_keep_the_margin(name):
    g = HMM["viterbi"][name]
    x, seg_off, model = H.viterbi_case(name)
    assert H.sha(x) == g["sha256"]
    count = {}
    states, margin = H.numpy_states(model, x, seg_off, with_margin=True, count=count)
    assert margin == g["margin"] and H.sha(states) == g["states_sha256"] and count == g["decisions"]
    if name in H.TIED:
        # every decision an exact tie (all four piece scores are the same bits): nothing to demand of a margin, but the path must
        # be all zeros - on the float64 model of the device's pieces first
        import hmm_piece_model as PM
        assert margin == 0.0 and count["finite"] > 0 and not states.any()
        for a, b in zip(seg_off[:-1].tolist(), seg_off[1:].tolist()):
            assert not any(PM.viterbi(x[a:b], model)), (a, b)
    else:
        assert margin > H.MARGIN                    # every FINITE decision; a pair of -inf candidates is a tie to the lower state
    if name in H.HARD_MODELS:
        lens = np.diff(seg_off).tolist()
        assert lens == [H.VIT_STEPS - 1, H.VIT_STEPS, H.VIT_STEPS + 1, 2 * H.VIT_STEPS + 1, 5 * H.VIT_STEPS, 0]
    if name == "forbidden":                         # 0 -> 1 cannot happen: one -inf candidate at every step, and a path that uses both states
        assert count["one_neg_inf"] > 0 and count["finite"] > 0 and 0 < int(states.sum()) < states.size
        assert all(np.all(np.diff(states[a:b].astype(int)) <= 0) for a, b in zip(seg_off[:-1].tolist(), seg_off[1:].tolist()))
    if name == "absorbing_start":                   # state 0 is never reachable: both of its candidates are -inf at every step
        assert count["two_neg_inf"] > 0 and states.all()
    if name in ("cuts", "forbidden"):               # the float64 model of the device's pieces gives the numpy path
        import hmm_piece_model as PM
        for a, b in zip(seg_off[:-1].tolist(), seg_off[1:].tolist()):
            assert PM.viterbi(x[a:b], model) == states[a:b].tolist(), (a, b)
    assert np.array_equal(states, H.model_of(model, True).predict_segments(x, seg_off))      # host-native agrees


def test_long_viterbi_input_regenerates():
    """(its 600 k-step margin is measured when the golden is made: tools/make_golden_update.py asserts it)"""
    g = HMM["viterbi"]["long_segment"]
    x, seg_off, model = H.viterbi_case("long_segment")
    assert H.sha(x) == g["sha256"] and g["margin"] > H.MARGIN and 0.2 < g["state1_fraction"] < 0.8
    states = H.model_of(model, True).predict_segments(x, seg_off)
    assert H.sha(states) == g["states_sha256"]


# ------------------------------------------------------------------------------------------------ the CLI on a fake engine
from fake_engine import FakeEngine  # noqa: E402


class _Engine(FakeEngine):
    """FakeEngine with the few members of Engine that HotPath touches besides."""

    def __init__(self, kmin, kmax, device=0):
        super().__init__(kmin, kmax)
        self.tiles = None

    @property
    def seq_lens(self):
        return [e.n for e in self.seqs]

    def scan(self, w, inc, rip=False, scaffolds_all=False, debug=False, pinned=False):
        return super().scan(w, inc, rip=rip, scaffolds_all=scaffolds_all)

    def profile_set(self, sym, tl, ex, nn):
        self.profile = (np.asarray(sym, dtype=np.int64), (tl, ex, nn))

    def close(self):
        pass


@pytest.fixture
def fake_cli(monkeypatch):
    from frisk_amd import cli, hotpath
    monkeypatch.setattr(hotpath, "Engine", _Engine)
    real_init = hotpath.HotPath.__init__

    def init(self, kMin, kMax, device=0, cache_dir=None, use_cache=True):
        real_init(self, kMin, kMax, device=device, cache_dir=None, use_cache=use_cache)      # (no packed-sequence cache: no device)
    monkeypatch.setattr(hotpath.HotPath, "__init__", init)
    made = []

    def model(device):
        made.append(device)
        return GaussianHMM2(native=True)         # the host-native model stands in for the device one
    monkeypatch.setattr(cli, "_fine_model", model)
    return cli, made


FA = os.path.join(GOLD, "inputs", "markov_islands.fa")


def _run(cli, tmp_path, sub, extra):
    out = tmp_path / sub
    argv = ["-H", FA, "-k", "4", "-w", "400", "-i", "150", "-t", str(out), "-F", "0.045", "--gffOutfile", "a.gff3",
            "--hmmOutfile", "states.gff3"] + extra
    assert cli.main(argv) == 0
    return out


def test_cli_updateHMM_writes_the_two_new_files_and_changes_nothing_else(fake_cli, tmp_path, capsys, caplog):
    from frisk_amd.hmm import hmm2BED, hmmBED2GFF
    cli, made = fake_cli
    plain = _run(cli, tmp_path, "P", [])
    plain_out = capsys.readouterr().out
    args = cli.mainArgs(["-H", FA, "--updateHMM"])
    assert args.updateHMM and not any(opt.startswith("update") for opt, _why in cli.unavailable(args))
    with caplog.at_level(logging.INFO, logger="frisk"):
        upd = _run(cli, tmp_path, "U", ["--updateHMM", "--updateWin", "200", "--updateInc", "100"])
    assert capsys.readouterr().out == plain_out                                     # the fine table is not echoed
    assert made == [0]
    fine_name, refined_name = "updateWin_200_inc_100_states.gff3", "HMMupdated_a.gff3"
    assert sorted(set(os.listdir(upd)) - set(os.listdir(plain))) == sorted([refined_name, fine_name])
    for f in os.listdir(plain):
        if not f.endswith(".p"):
            assert open(upd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not any("_window_200_" in f for f in os.listdir(upd))                   # the fine table is not cached
    # the fine track is hmm2BED on a fine table of the same engine; the refined file is refineAnomalies on the two
    from frisk_amd.hotpath import HotPath
    hp = HotPath(1, 4)
    try:
        a = cli.mainArgs(["-H", FA, "-k", "4", "-w", "200", "-i", "100"])
        hp.genomeProfile(a)
        fine_table, _ = hp.scanTable(a, FA)
    finally:
        hp.close()
    intervals, _m = hmm2BED(fine_table, GaussianHMM2(native=True))
    assert open(upd / fine_name).read() == "".join(hmmBED2GFF(intervals)) and len(intervals) > 2
    coarse = [ln.rstrip("\n").split("\t") for ln in open(upd / "a.gff3") if not ln.startswith("#")]
    fine_rows = [ln.rstrip("\n").split("\t") for ln in open(upd / refined_name) if not ln.startswith("#")]
    assert len(coarse) == len(fine_rows) > 0
    anomalies = [(c[0], int(c[3]), int(c[4])) for c in coarse]
    want, kept = pp.refineAnomalies(intervals, anomalies, emit=lambda s: None)
    assert [(r[0], int(r[3]), int(r[4])) for r in fine_rows] == [tuple(w) for w in want]
    bounds = {int(v) for i in intervals for v in i[1:3]}
    changed = 0
    for c, r in zip(coarse, fine_rows):
        assert c[:3] == r[:3] and c[5:] == r[5:]                                    # every other field carried through
        for k in (3, 4):
            if c[k] != r[k]:
                changed += 1
                assert int(r[k]) in bounds
    assert changed > 0 and kept < len(coarse)
    assert any(r.getMessage().startswith("Refined") for r in caplog.records)
    # both caches hit: the sequence is loaded again for the fine scan, same two files
    before = {f: open(upd / f, "rb").read() for f in (fine_name, refined_name)}
    for f in before:
        os.remove(upd / f)
    _run(cli, tmp_path, "U", ["--updateHMM", "--updateWin", "200", "--updateInc", "100"])
    assert {f: open(upd / f, "rb").read() for f in before} == before


def test_cli_updateHMM_is_skipped_with_a_warning(fake_cli, tmp_path, caplog):
    cli, made = fake_cli
    with caplog.at_level(logging.WARNING, logger="frisk"):
        out = _run(cli, tmp_path, "E", ["--updateHMM", "--updateWin", "200", "--updateInc", "100", "--exitAfter", "WindowKLD"])
    assert made == [] and not any(f.startswith(("updateWin_", "HMMupdated_")) for f in os.listdir(out))
    assert any("--updateHMM skipped" in r.getMessage() for r in caplog.records)


def test_cli_updateHMM_fine_zero_division_is_skipped(fake_cli, tmp_path, caplog, monkeypatch):
    """A fine scan that meets the reference's ZeroDivisionError: a warning, no refined file, every other output as without."""
    from frisk_amd import hotpath
    cli, made = fake_cli
    real = hotpath.HotPath.scanTable

    def scanTable(self, args, querySeq, debug=False):
        if args.windowlen == 200:
            raise ZeroDivisionError("float division by zero")
        return real(self, args, querySeq, debug=debug)
    monkeypatch.setattr(hotpath.HotPath, "scanTable", scanTable)
    with caplog.at_level(logging.WARNING, logger="frisk"):
        out = _run(cli, tmp_path, "Z", ["--updateHMM", "--updateWin", "200", "--updateInc", "100"])
    assert made == [] and os.path.isfile(out / "a.gff3")
    assert not any(f.startswith(("updateWin_", "HMMupdated_")) for f in os.listdir(out))
    assert any("ZeroDivisionError" in r.getMessage() for r in caplog.records)
