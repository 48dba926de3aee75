"""The device E step (csrc/hmm_kernels.h through frisk_hmm_estep_gpu - the code a round of frisk_hmm_fit_gpu runs) against the
extended-precision oracle (tests/hmm_oracle_hp.py), driven with CHOSEN models: transition probabilities of 1e-30 and 1e-70, a
variance of 1e-8, an absorbing state, equal states, emissions that underflow to exactly 0 on both sides of a cut, the forward
walk's flush below 1e-200; sizes around every layout change (one piece / two, the host form's first cut, the cap P == PIECES).
Everything the comparison rests on comes from the CPU (tests/hmm_estep_cases.py, tests/golden/hmm_estep.json, qualified in
tests/test_hmm_estep_cpu.py): the tolerance is 8 x the largest error against the oracle of a float64 model of the device's piece
scheme and of the host-native form, per quantity over the whole case set - never a number the device produced."""
import numpy as np
import pytest

import hmm_estep_cases as E
import hmm_gpu_cases as H
import hmm_piece_model as PM
from frisk_amd.hmm import GaussianHMM2
from test_hmm_estep_cpu import m_step

pytestmark = pytest.mark.gpu

G = E.golden()
PAIRS = [(m, f) for m in E.MODELS for f in E.FAMILIES]


def device_e_step(model, x):
    return H.model_of(E.MODELS[model], "gpu").e_step(x)


@pytest.mark.parametrize("model,family", PAIRS)
def test_device_estep_against_the_oracle_window_by_window(model, family):
    for n in E.SMALL:
        x = E.case_input(model, family, n)
        assert H.sha(x) == G["cases"][E.case_id(model, family, n)]["sha256"]
        got = device_e_step(model, x)
        _e, msg = E.check(model, family, n, got)
        print(msg)
        E.structure(n, got)
        again = device_e_step(model, x)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "second call differs: " + E.case_id(model, family, n)


@pytest.mark.parametrize("model,family", PAIRS)
def test_device_estep_against_the_recorded_oracle_around_the_host_cut_and_the_cap(model, family):
    for n in E.LARGE:
        x = E.case_input(model, family, n)
        assert H.sha(x) == G["cases"][E.case_id(model, family, n)]["sha256"]
        got = device_e_step(model, x)
        _e, msg = E.check(model, family, n, got)
        print(msg)
        E.structure(n, got)
        again = device_e_step(model, x)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "second call differs: " + E.case_id(model, family, n)


def device_cov_sums(sq):
    """hmm_covar_walk + hmm_reduce_rows: every device piece added window by window, then the pieces in the fixed order."""
    n = sq.shape[0]
    cut = PM.bounds(n, PM.pieces_of(n))
    out = []
    for j in (0, 1):
        col, rows = sq[:, j].tolist(), []
        for a, b in zip(cut[:-1], cut[1:]):
            s = 0.0
            for v in col[a:b]:
                s += v
            rows.append(s)
        out.append(PM._reduce_rows(rows))
    return np.array(out)


@pytest.mark.parametrize("name", ["clean", "outlier", "n2"])
def test_the_hook_is_the_fit_device(name):
    """fit(n_iter=1) == hmm.py's M step applied to e_step under the start model (fit(n_iter=0)), bit for bit."""
    x = H.fit_input(name)
    start = GaussianHMM2(native="gpu", n_iter=0).fit(x)
    post, stats, ll = start.e_step(x)
    one = GaussianHMM2(native="gpu", n_iter=1).fit(x)
    assert one.n_iter_ == 1 and one.loglik_ == ll
    for got, want in zip((one.means_, one.covars_, one.startprob_, one.transmat_), m_step(x, post, stats, device_cov_sums)):
        assert np.array_equal(np.asarray(got), np.asarray(want)), name


def test_device_estep_without_posteriors_and_bad_arguments():
    import ctypes as C
    from frisk_amd import _ffi
    x = E.case_input("kld", "regimes", 97)
    m = H.model_of(E.MODELS["kld"], "gpu")
    post, stats, ll = m.e_step(x)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    pars = [np.ascontiguousarray(a, dtype=np.float64) for a in (m.means_, m.covars_, m.startprob_, np.ravel(m.transmat_))]
    only = np.zeros(9)
    assert _ffi.lib().frisk_hmm_estep_gpu(0, p(x), x.size, p(pars[0]), p(pars[1]), p(pars[2]), p(pars[3]), None, p(only)) == _ffi.OK
    assert np.array_equal(only[:8], stats) and only[8] == ll
    with pytest.raises(ValueError):
        m.e_step(np.array([0.1, float("inf")]))
    with pytest.raises(_ffi.FriskHipError):
        H.model_of(E.MODELS["kld"], "gpu", device=1 << 20).e_step(x)
