"""The two ends of the device fit (csrc/hmm_kernels.h through frisk_hmm_fit_gpu) against the extended-precision oracle
(tests/hmm_oracle_hp.py): the deterministic start - hmm_init_range, hmm_init_range_final, hmm_init_assign, hmm_init_var and
hmm_reduce_rows, through GaussianHMM2(native="gpu", n_iter=0) - at every size at which the chunk layout of either form changes
(C = 1 -> 2 -> 3, the cap C = 1024, chunks of 256 and 257 windows interleaved, the host's 4096-window pieces), and the model after one
and after three EM rounds from that start (hmm_covar_walk and the M step behind the E step) at every size at which the E step's
piece layout changes.  Everything the comparison rests on comes from the CPU (tests/hmm_start_cases.py, tests/golden/hmm_start.json,
qualified in tests/test_hmm_start_cpu.py): inputs regenerate to a recorded sha256, and a tolerance is 8 x the largest error against
the oracle of the numpy specification, a float64 model of the device's layout and the host-native library, per quantity over the
whole case set - never a number the device produced.  The round comparisons are held, besides, to the same multiple of the two forms
that work in scaled space (S.check_device_rounds says why)."""
import numpy as np
import pytest

import hmm_gpu_cases as H
import hmm_start_cases as S
import hmm_start_model as SM

pytestmark = pytest.mark.gpu

G = S.golden()


@pytest.mark.parametrize("family", S.FAMILIES)
def test_device_start_against_the_oracle_at_every_chunk_edge(family):
    for n in S.SIZES:
        x = S.start_input(family, n)
        assert H.sha(x) == G["start_cases"][S.start_id(family, n)]["sha256"]
        m, got = S.fit_start(x, "gpu")
        _e, msg = S.check_start(family, n, got)
        print(msg)
        assert m.n_iter_ == 0 and m.loglik_ == -np.inf
        assert m.means_[0] <= m.means_[1] and m.covars_[0] == m.covars_[1]
        assert np.array_equal(m.startprob_, [0.5, 0.5]) and np.array_equal(m.transmat_, [[0.5, 0.5], [0.5, 0.5]])
        again = S.fit_start(x, "gpu")[1]
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), "second call differs: " + S.start_id(family, n)
        if family == "constant":
            assert got[0].tolist() == [0.1, 0.1] and got[1].tolist() == [S.MIN_COVAR, S.MIN_COVAR]
        if family == "two_values" and n > 1:
            assert got[0].tolist() == [0.03, 0.15]
        if family.startswith("edges") and n > 1:
            assert got[0].tolist() == [S.EDGE_MIN, S.EDGE_MAX]


@pytest.mark.parametrize("family", ["regimes", "overlap", "ties", "offset"])
def test_device_start_is_the_model_of_its_layout_bit_for_bit(family):
    """No transcendental function and no fused operation: the float64 model of the chunk scheme (the one the tolerance was measured
    on) is the device's result itself - up to 8193 windows, and at the cap."""
    for n in S.SMALL + (262144, 262144 + 1023):
        x = S.start_input(family, n)
        means, covar, _r = SM.start(x, "device")
        got = S.fit_start(x, "gpu")[1]
        assert got[0].tolist() == means and got[1].tolist() == [covar, covar], (family, n, got, means, covar)


@pytest.mark.parametrize("family", S.ROUND_FAMILIES)
def test_device_rounds_against_the_oracle_at_every_piece_layout_edge(family):
    for n in S.ROUND_SIZES:
        x = S.round_input(family, n)
        assert H.sha(x) == G["round_cases"][S.round_id(family, n)]["sha256"]
        for r in S.ROUNDS:
            m, got = S.fit_rounds(x, r, "gpu")
            _e, msg = S.check_device_rounds(family, n, r, got)
            print(msg)
            assert m.n_iter_ == r and m.means_[0] <= m.means_[1]
            assert S.fit_rounds(x, r, "gpu")[1] == got, "second call differs: %s after %d rounds" % (S.round_id(family, n), r)
        # n_iter = 1 with the default tol is the same single round (the first round tests no gain)
        one = H.GaussianHMM2(native="gpu", n_iter=1).fit(x)
        assert (H.params(one), one.loglik_) == S.fit_rounds(x, 1, "gpu")[1]
