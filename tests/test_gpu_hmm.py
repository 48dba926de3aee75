"""The 2-state Gaussian HMM on the device (csrc/hmm_kernels.h: frisk_hmm_fit_gpu / frisk_hmm_viterbi_gpu) and --updateHMM end to
end.  The inputs, the tolerance and the conditions under which equality may be demanded come from the CPU
(tests/hmm_gpu_cases.py, tests/golden/hmm_gpu.json, qualified in tests/test_update_hmm_cpu.py): the tolerance of the fit is 8 x
the spread between the numpy specification and the host-native fit on these same inputs; the round counts must be equal (no
round's gain is within 1e-6 of tol); the Viterbi states must be identical, no window exempted (the numpy path decides every step
by more than 1e-9)."""
import json
import os

import numpy as np
import pytest

import hmm_gpu_cases as H
from frisk_amd.hmm import GaussianHMM2

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HMM = json.load(open(os.path.join(GOLD, "hmm_gpu.json")))
TOL = HMM["tolerance"]


@pytest.mark.parametrize("name", list(H.FIT_CASES))
def test_device_fit_equals_the_specification_and_the_host(name):
    g = HMM["fit"][name]
    x = H.fit_input(name)
    assert H.sha(x) == g["sha256"]
    dev = GaussianHMM2(native="gpu").fit(x)
    host = GaussianHMM2(native=True).fit(x)
    assert dev.n_iter_ == host.n_iter_ == g["numpy"]["n_iter_"]
    vs_numpy = H.spread(g["numpy"], H.params(dev), g["numpy"]["loglik_"], dev.loglik_)
    vs_host = H.spread(H.params(host), H.params(dev), host.loglik_, dev.loglik_)
    print("%s: device against numpy %.3g, against host-native %.3g (allowed %.3g = 8 x %.3g)"
          % (name, vs_numpy, vs_host, TOL, HMM["spread_numpy_host"]))
    assert vs_numpy <= TOL and vs_host <= TOL
    assert dev.means_[0] <= dev.means_[1] and abs(dev.startprob_.sum() - 1) < 1e-12
    assert np.max(np.abs(dev.transmat_.sum(axis=1) - 1)) < 1e-12
    # bit-identical from run to run
    again = GaussianHMM2(native="gpu").fit(x)
    assert again.loglik_ == dev.loglik_ and again.n_iter_ == dev.n_iter_
    for f in H.FIELDS:
        assert np.array_equal(getattr(again, f), getattr(dev, f)), f


@pytest.mark.parametrize("native", ["gpu"])
def test_one_em_round_equals_the_closed_form_on_exact_posteriors(native):
    """tests/test_hmm_cpu.py's check of the host forms, for the device: fit(n_iter=1) from the deterministic start == the M step
    on the enumerated posteriors (hmmlearn's default priors); three rounds == the closed form applied three times."""
    from oracle import hmm_exhaustive as X
    rng = np.random.default_rng(31)
    for c in range(25):
        n = int(rng.integers(3, 13))
        regime = (np.arange(n) * 3 // n) % 2
        x = np.where(regime == 0, rng.normal(0.04, 0.01, n), rng.normal(0.15, 0.04, n))
        init = GaussianHMM2(native=False)
        init._init(x)
        p = (init.means_.tolist(), init.covars_.tolist(), init.startprob_.tolist(), init.transmat_.tolist())
        for rounds in (1, 3):
            q, ll = p, None
            for _ in range(rounds):
                nm, nc, ns, nt, ll = X.em_step(x.tolist(), *q)
                q = (nm, nc, ns, nt)
            m = GaussianHMM2(n_iter=rounds, tol=-1e300, native=native).fit(x)
            assert m.n_iter_ == rounds
            assert abs(m.loglik_ - ll) <= 1e-10 * max(1.0, abs(ll))
            for got, want in zip((m.means_, m.covars_, m.startprob_, m.transmat_), q):
                assert np.max(np.abs(np.ravel(got) - np.ravel(np.array(want)))) <= 1e-10 * max(1.0, float(np.max(np.abs(want)))), (c, rounds)


def test_device_fit_rejects_what_the_host_rejects():
    with pytest.raises(ValueError):
        GaussianHMM2(native="gpu").fit(np.array([0.1, float("nan")]))
    with pytest.raises(ValueError):
        GaussianHMM2(native="gpu").fit(np.array([]))
    zero = GaussianHMM2(native="gpu", n_iter=0).fit(np.array([0.1, 0.3, 0.2]))
    host = GaussianHMM2(native=True, n_iter=0).fit(np.array([0.1, 0.3, 0.2]))
    assert zero.n_iter_ == 0 and np.allclose(zero.means_, host.means_, rtol=0, atol=1e-15) and np.allclose(zero.covars_, host.covars_, rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", list(H.VITERBI_CASES))
def test_device_viterbi_states_are_the_numpy_path(name):
    g = HMM["viterbi"][name]
    x, seg_off, model = H.viterbi_case(name)
    assert H.sha(x) == g["sha256"] and (g["margin"] > H.MARGIN or (name in H.TIED and g["margin"] == 0.0))
    want = H.numpy_states(model, x, seg_off)                    # the specification, recomputed (one Python step per window)
    assert H.sha(want) == g["states_sha256"]                    # ... and it is the path whose margin was measured
    got = H.model_of(model, "gpu").predict_segments(x, seg_off)
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert np.array_equal(got, H.model_of(model, "gpu").predict_segments(x, seg_off))
    if name == "symmetric":                     # exact ties at every step and at every cut: the lower state throughout
        assert not got.any()
    elif name == "absorbing_start":             # state 0 unreachable (-inf on both of its candidates, in every piece and at every cut)
        assert got.all()
    elif x.size > 100:
        assert 0 < int(got.sum()) < got.size


def test_device_viterbi_edges():
    m = H.model_of(H.KLD_MODEL, "gpu")
    assert m.predict(np.array([])).size == 0
    assert m.predict_segments(np.array([]), [0, 0, 0]).size == 0
    assert m.predict(np.array([0.04])).tolist() == [0] and m.predict(np.array([0.2])).tolist() == [1]
    # a slice of a longer array: segments need not start at 0
    x, seg_off, model = H.viterbi_case("cuts")
    full = m.predict_segments(x, seg_off)
    part = np.zeros_like(full)
    for lo in range(0, seg_off.size - 1, 4):
        sub = seg_off[lo:lo + 5]
        part[sub[0]:sub[-1]] = m.predict_segments(x, sub)[sub[0]:sub[-1]]
    assert np.array_equal(part, full)
    # a transition that cannot happen (log 0) and ties: the lower state, as numpy.argmax
    hard = dict(means=[0.0, 0.0], covars=[1.0, 1.0], start=[0.5, 0.5], trans=[[1.0, 0.0], [0.5, 0.5]])
    xs = np.linspace(-1, 1, 200)                 # (one piece: operation for operation the host form)
    assert np.array_equal(H.model_of(hard, "gpu").predict(xs), H.model_of(hard, False)._predict_py(xs))


# --------------------------------------------------------------------------------------------------------- --updateHMM, CLI
def test_cli_updateHMM_end_to_end(tmp_path, capsys):
    from golden_util import Case
    from frisk_amd import Engine, postprocess as pp
    from frisk_amd.cli import main
    from frisk_amd.hmm import hmm2BED, hmmBED2GFF
    from frisk_amd.table import ScoreTable
    from frisk_amd import _ffi
    c = Case("markov_k6")
    g = json.load(open(os.path.join(GOLD, "writers.json")))["e2e"]["markov_k6"]
    base = ["-H", c.host, "-k", "6", "-w", "400", "-i", "150", "-F", str(g["forceThresholdKLD"]), "--mergeDist", str(g["mergeDist"]),
            "--gffOutfile", "a.gff3", "--hmmOutfile", "states.gff3"]
    assert main(base + ["-t", str(tmp_path / "P")]) == 0
    plain_out = capsys.readouterr().out
    assert main(base + ["-t", str(tmp_path / "U"), "--updateHMM", "--updateWin", "200", "--updateInc", "100"]) == 0
    assert capsys.readouterr().out == plain_out
    P, U = tmp_path / "P", tmp_path / "U"
    for f in ("a.gff3", "raw_window_scores.bed"):
        assert open(U / f, "rb").read() == open(P / f, "rb").read(), f
    new = sorted(set(os.listdir(U)) - set(os.listdir(P)))
    assert new == ["HMMupdated_a.gff3", "updateWin_200_inc_100_states.gff3"]
    # the fine track == hmm2BED with the HOST-native model on a fine table from Engine.scan
    from frisk_amd.fasta import readFasta
    names, seqs = readFasta(c.host)
    with Engine(1, 6) as e:
        e.load(seqs)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        res = e.scan(200, 100)
    kept = np.nonzero(res.kept)[0]
    assert not np.any(res.status[kept] & _ffi.ROW_ZERO_WEIGHT)
    int0 = ((res.status[kept] & _ffi.ROW_NO_MAXMER) != 0).astype(np.uint8)
    fine = ScoreTable(names, res.seq_index[kept], res.start[kept], res.stop[kept], res.kld[kept], res.gc[kept], None, None, None, int0)
    intervals, _m = hmm2BED(fine, GaussianHMM2(native=True))
    assert open(U / "updateWin_200_inc_100_states.gff3").read() == "".join(hmmBED2GFF(intervals)) and len(intervals) > 2
    coarse = [ln.rstrip("\n").split("\t") for ln in open(U / "a.gff3") if not ln.startswith("#")]
    refined = [ln.rstrip("\n").split("\t") for ln in open(U / "HMMupdated_a.gff3") if not ln.startswith("#")]
    anomalies = [(r[0], int(r[3]), int(r[4])) for r in coarse]
    want, kept_as_is = pp.refineAnomalies(intervals, anomalies, emit=lambda s: None)
    snapped = pp.updateHMM(intervals, anomalies)
    assert len(refined) == len(coarse) > 0
    bounds = {int(v) for i in intervals for v in i[1:3]}
    changed = 0
    for r, w, s, a, co in zip(refined, want, snapped, anomalies, coarse):
        assert (r[0], int(r[3]), int(r[4])) == tuple(w)
        assert tuple(w) == ((s[0], int(s[1]), int(s[2])) if int(s[1]) < int(s[2]) else a)     # pp.updateHMM applied to those
        assert r[:3] == co[:3] and r[5:] == co[5:]
        for k in (3, 4):
            if r[k] != co[k]:
                changed += 1
                assert int(r[k]) in bounds                      # every changed boundary is a boundary of the fine track
    assert changed > 0
