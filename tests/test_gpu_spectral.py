"""Spectral clustering on the GPU (csrc/spectral_kernels.h through frisk_amd.projection.Spectral / spectral_embedding / spectral),
per golden case of tests/golden/spectral.json (sklearn's results, tools/make_golden_spectral.py): the affinities, degrees and
products against long double (tests/spectral_oracle_hp.py) within bounds of the rounding they carry, M against scipy's formula
on the device's own A0 and dd, the embedding against sklearn's as a subspace (Davis-Kahan) and in its rows' pairwise distances,
the labels as a partition, bit-reproducibility, the argument checks of the C ABI, and the CLI end to end.

Measured on an MI355X: the device's exp uses at most 0.249 of C_EXP = 4 (printed by test_affinity); 34-39 iterations to residuals of
5.6e-11 .. 9.9e-11 (1 iteration where p = n); subspace sine 0.19 .. 0.95 of its bound (printed by test_embedding).  DESIGN.md section
9.5 has the timings."""
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import spectral_oracle as SO
import spectral_oracle_hp as HP
from golden_util import INPUTS

pytestmark = pytest.mark.gpu

G = SO.golden()
CASES = sorted(G["cases"])
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LD = np.longdouble
EPS = SO.EPS


@functools.lru_cache(maxsize=None)
def device(case):
    """(A0, dd, n_isolated, M) of one handle on the case's Y: computed once, read-only."""
    from frisk_amd.projection import Spectral
    with Spectral(SO.array(case, "Y"), G["cases"][case]["gamma"]) as h:
        M = h.matrix()
        A0 = h.affinity()
        dd, iso = h.degrees()
        assert h.matrix().tobytes() == M.tobytes()          # the affinities on request leave the same M behind
    for a in (A0, dd, M):
        a.setflags(write=False)
    return A0, dd, iso, M


@functools.lru_cache(maxsize=None)
def reference(case):
    """(A_hp, d2_hp, the allowance of |A0 - A_hp|) in long double / float64."""
    g = G["cases"][case]
    A_hp, d2 = HP.affinity(SO.array(case, "Y"), g["gamma"])
    return A_hp, d2, HP.affinity_bound(A_hp, d2, g["d"], g["gamma"])


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("case", CASES)
def test_affinity(case):
    """A0 exactly symmetric with an exactly zero diagonal; |A0 - A_hp| <= ((d + 2) gamma d2 + C_EXP) eps64 A_hp, anything in
    [0, DBL_MIN] where the exact value is below the smallest normal double"""
    g = G["cases"][case]
    A0 = device(case)[0]
    A_hp, d2, bound = reference(case)
    assert np.array_equal(A0, A0.T) and np.all(np.diagonal(A0) == 0.0)
    assert np.all(A0 >= 0.0) and np.all(A0 <= 1.0)
    err = np.abs(A0.astype(LD) - A_hp).astype(np.float64)
    normal = A_hp >= LD(HP.DBL_MIN)
    excess = err[normal] / (EPS * A_hp[normal].astype(np.float64)) - (g["d"] + 2) * g["gamma"] * d2[normal].astype(np.float64)
    print("%s: worst device ratio of exp %.3f (C_EXP %.0f)" % (case, float(excess.max(initial=0.0)), HP.C_EXP))
    assert np.all(err <= bound), (case, float((err / bound)[bound > 0].max()))
    assert np.all(A0[~normal] <= HP.DBL_MIN)


@pytest.mark.parametrize("case", CASES)
def test_degrees(case):
    """|w - w_hp| <= (n + 1) eps64 w_hp + the summed affinity bounds, dd = sqrt(w) one rounding more; a column whose every exact
    affinity is below half the smallest subnormal is isolated: dd == 1 exactly, and counted"""
    g = G["cases"][case]
    n = g["n"]
    _A0, dd, iso, _M = device(case)
    A_hp, _d2, bound = reference(case)
    certain_zero = np.all(A_hp < LD(2.0) ** -1075, axis=0)
    assert iso == g["n_isolated"] == int(certain_zero.sum())
    assert np.all(dd[certain_zero] == 1.0)
    w_hp = HP.degrees(A_hp)[~certain_zero]
    assert np.all(w_hp > LD(HP.DBL_MIN) * n)                    # no golden column sits between the two regimes
    rel = ((n + 1) * EPS * w_hp + bound[:, ~certain_zero].sum(axis=0).astype(LD)) / w_hp
    want = np.sqrt(w_hp)
    err = np.abs(dd[~certain_zero].astype(LD) - want)
    assert np.all(err <= (rel / 2 + rel * rel + EPS) * want), case


@pytest.mark.parametrize("case", CASES)
def test_matrix(case):
    """M against scipy's (A0 / dd) / dd[:, None] in numpy from the device's own A0 and dd: equal or 1 ulp apart per entry (equal
    wherever scipy's entry and its mirror are), and exactly symmetric"""
    A0, dd, _iso, M = device(case)
    S = SO.scipy_matrix(A0, dd)
    assert np.array_equal(M, M.T)
    assert np.all(np.abs(M - S) <= np.spacing(np.minimum(np.abs(M), np.abs(S)))), case
    same = S == S.T
    assert np.array_equal(M[same], S[same])
    assert np.array_equal(M, SO.matrix(A0, dd))                 # the mean of the entry and its mirror, bit for bit


@pytest.mark.parametrize("case", CASES)
def test_product(case):
    """Z = M Q against the long-double product of the device's own M: |Z - Z_hp| <= (n + 2) eps64 |M| |Q|, for random Q and Q
    with columns scaled by +-1e+-150, at p = 1, k and 26; the same bytes from a second handle and a second call"""
    from frisk_amd.projection import Spectral
    g = G["cases"][case]
    n, k = g["n"], g["k"]
    M = device(case)[3]
    rs = np.random.RandomState(g["seed"] + 100)
    Y = SO.array(case, "Y")
    with Spectral(Y, g["gamma"]) as h, Spectral(Y, g["gamma"]) as h2:
        for p in sorted({1, k, 26}):
            scale = np.array([1e150, -1e-150, 1.0, -1e150, 1e-150] * 6)[:p]
            for Q in (rs.normal(size=(n, p)), rs.normal(size=(n, p)) * scale):
                Z = h.mq(Q)
                assert Z.tobytes() == h2.mq(Q).tobytes() == h.mq(Q).tobytes()
                err = np.abs(Z.astype(LD) - HP.product(M, Q)).astype(np.float64)
                assert np.all(err <= (n + 2) * EPS * (np.abs(M) @ np.abs(Q))), (case, p)
        assert h.last_ms()[2] > 0.0
        # the documented summation order is that of the NMF product X Q (lane l: columns l, l + 64, ...; then the wave butterfly),
        # which takes any non-negative X: on the device's own M it gives the same bits
        from frisk_amd.projection import NMF
        with NMF(M, 1) as x:
            for p in sorted({1, k, 26}):
                Q = rs.normal(size=(n, p))
                assert h.mq(Q).tobytes() == x.xq(Q).tobytes(), (case, p)


# ------------------------------------------------------------------------------------------------ embedding and labels
@pytest.mark.parametrize("case", CASES)
def test_embedding(case):
    """residuals <= tol; eigenvalues within residual + n eps64 of the golden's; the subspace within (r_ours + r_golden) / gap_k +
    n eps64 of sklearn's, both residuals from the host M; the rows' pairwise distances within that times 2 max(1 / dd)"""
    from frisk_amd import projection as P
    g = G["cases"][case]
    with P.Spectral(SO.array(case, "Y"), g["gamma"]) as h:
        E, lam, res, it = P.spectral_embedding(h, g["k"], g["seed"])
        t = h.timings
    assert res.max() <= P.SPECTRAL_TOL and it < P.SPECTRAL_MAX_ITER and t["products"] == it and t["product_ms"] > 0
    _A, dd, M = SO.host_matrix(case)
    ratio = SO.check_embedding(case, E, lam, res, M, dd)
    print("%s: %d iterations, residual %.3g, sine / bound %.3f" % (case, it, res.max(), ratio))


@pytest.mark.parametrize("case", CASES)
def test_labels_and_reproducibility(case):
    """spectral() gives sklearn's partition, renumbered by first occurrence, and the same bytes twice"""
    from frisk_amd import projection as P
    g = G["cases"][case]
    Y = SO.array(case, "Y")
    a, b = P.spectral(Y, g["k"], seed=g["seed"], gamma=g["gamma"]), P.spectral(Y, g["k"], seed=g["seed"], gamma=g["gamma"])
    assert a.labels.dtype == np.int32 and a.labels.tolist() == SO.renumber(a.labels).tolist()
    assert SO.same_partition(a.labels, SO.array(case, "labels")), case
    assert a.n_isolated == g["n_isolated"] and a.embedding.shape == (g["n"], g["k"])
    assert a.labels.tobytes() == b.labels.tobytes() and a.embedding.tobytes() == b.embedding.tobytes()
    assert a.eigenvalues.tobytes() == b.eigenvalues.tobytes() and a.n_iter == b.n_iter
    assert set(a.timings) >= {"affinity_ms", "normalise_ms", "products_ms", "host_ms", "kmeans_ms"}


def test_isolated_point_logs_sklearns_warning(caplog):
    import logging
    from frisk_amd import projection as P
    g = G["cases"]["isolated"]
    with caplog.at_level(logging.WARNING):
        r = P.spectral(SO.array("isolated", "Y"), g["k"], seed=g["seed"])
    assert r.n_isolated == 1 and "Graph is not fully connected, spectral embedding may not work as expected." in caplog.text


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_argument_checks():
    from frisk_amd import _ffi
    L, E = _ffi.lib(), _ffi.E_ARG
    Y = np.random.RandomState(0).rand(20, 3)
    bad = Y.copy()
    bad[7, 1] = np.inf
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    h = C.c_void_p()
    assert L.frisk_spectral_create(0, p(Y), 20, 3, 1.0, None) == E
    assert L.frisk_spectral_create(0, None, 20, 3, 1.0, C.byref(h)) == E
    for n in (1, 0, 50001):
        assert L.frisk_spectral_create(0, p(Y), n, 3, 1.0, C.byref(h)) == E
    for d in (0, 65):
        assert L.frisk_spectral_create(0, p(Y), 20, d, 1.0, C.byref(h)) == E
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        assert L.frisk_spectral_create(0, p(Y), 20, 3, gamma, C.byref(h)) == E
    assert L.frisk_spectral_create(0, p(bad), 20, 3, 1.0, C.byref(h)) == E and not h.value
    assert L.frisk_spectral_create(0, p(Y), 20, 3, 1.0, C.byref(h)) == _ffi.OK and h.value
    try:
        out, Q, iso = np.empty((20, 26)), np.ones((20, 26)), C.c_int64()       # room for A0 (20 x 20) and for Z (20 x 26)
        assert L.frisk_spectral_affinity(h, None) == E and L.frisk_spectral_affinity(None, p(out)) == E
        assert L.frisk_spectral_matrix(h, None) == E and L.frisk_spectral_matrix(None, p(out)) == E
        assert L.frisk_spectral_degrees(h, None, C.byref(iso)) == E and L.frisk_spectral_degrees(h, p(out), None) == E
        assert L.frisk_spectral_degrees(None, p(out), C.byref(iso)) == E
        for pp in (0, 27, -1):
            assert L.frisk_spectral_mq(h, p(Q), pp, p(out)) == E
        assert L.frisk_spectral_mq(h, None, 2, p(out)) == E and L.frisk_spectral_mq(h, p(Q), 2, None) == E
        assert L.frisk_spectral_mq(None, p(Q), 2, p(out)) == E
        assert L.frisk_spectral_last_ms(h, 3) == -1.0 and L.frisk_spectral_last_ms(None, 0) == -1.0
        assert L.frisk_spectral_mq(h, p(Q), 26, p(out)) == _ffi.OK and L.frisk_spectral_last_ms(h, 0) > 0.0
    finally:
        L.frisk_spectral_destroy(h)
    L.frisk_spectral_destroy(None)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_spectral_dumps_its_labels(tmp_path):
    """--cluster SPECTRAL --kClusters 3 --dumpPCAdata on the fixture: anomSPECTRAL holds P.spectral of the PCA projection of the
    dumped proportions, the unavailable warning is still printed, and no cluster GFF3 is written"""
    import json
    from frisk_amd import projection as P
    e = json.load(open(os.path.join(SO.GOLD, "projection_cluster.json")))["e2e"]
    out = tmp_path / "T"
    argv = list(e["argv"])
    argv[argv.index("DBSCAN")] = "SPECTRAL"
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(INPUTS, e["fasta"]), "-t", str(out)] + argv + [
        "--kClusters", "3", "--dumpPCAdata"]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "--cluster is not available in this build" in p.stderr and "SPECTRAL of %d points" % e["n_anomalous"] in p.stderr
    assert [f for f in os.listdir(out) if "cluster_labeled" in f] == []
    counts = pickle.load(open(out / "anomCounts", "rb"))
    labels = pickle.load(open(out / "anomSPECTRAL", "rb"))
    want = P.spectral(P.pca(counts, 2).Y, 3, seed=0)
    assert labels.dtype == np.int32 and labels.shape == (e["n_anomalous"],) and labels.tobytes() == want.labels.tobytes()
