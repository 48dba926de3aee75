"""PY-TSNE on the GPU (csrc/tsne_kernels.h through frisk_amd.projection.TSNE / tsne): affinities and single optimiser steps
against the reference's own recorded states (tests/golden/tsne, tools/make_golden_tsne.py) within the forward-error bounds of
tests/tsne_oracle.py, full runs against the reference's ensembles, determinism and resumability, tile and block edges against
the oracle, argument checks of the C ABI, one run at n = 20 000, and the CLI end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tsne_oracle as TO
from golden_util import GOLD, INPUTS

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "tsne.json")))
CASES = sorted(G["cases"])
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def A(case):
    return np.load(os.path.join(GOLD, "tsne", G["cases"][case]["file"]))


def _handle(a, g, Y0=None):
    from frisk_amd.projection import TSNE
    return TSNE(a["Xp"], a["Y0"] if Y0 is None else Y0, g["perplexity"])


def _same_partition(a, b):
    if not np.array_equal(a == -1, b == -1):
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("case", CASES)
def test_affinities_match_reference(case):
    g, a = G["cases"][case], A(case)
    with _handle(a, g) as h:
        beta, tries, q = h.affinities(q=True)
    assert tries.tolist() == a["tries"].tolist()
    assert np.all(np.abs(beta - a["beta"]) <= 1e-12 * a["beta"])
    assert np.array_equal(q, q.T)
    if "q" in a:
        qg = a["q"]
        clamped = qg == TO.Q_FLOOR
        assert np.array_equal(q == TO.Q_FLOOR, clamped)
        tol = TO.q_tolerance(a["Xp"], a["beta"])
        assert np.all((np.abs(q - qg) <= tol * qg)[~clamped])


# ------------------------------------------------------------------------------------------------ single steps
@pytest.mark.parametrize("case", CASES)
def test_steps_match_reference_snapshots(case):
    """set the reference's state at t, run(t, t + 1), compare with its state at t + 1 within the oracle's bound."""
    g, a = G["cases"][case], A(case)
    skipped = total = 0
    with _handle(a, g) as h:
        q = h.affinities(q=True)[2]
        qref = a["q"] if "q" in a else q
        q_rel = float(np.max(np.abs(q - qref) / qref))
        assert q_rel <= float(np.max(TO.q_tolerance(a["Xp"], a["beta"])))
        for t in g["snapshots"]:
            h.set(a["Y_%d" % t], a["iY_%d" % t], a["gains_%d" % t])
            cost = h.run(t, t + 1)
            Y, iY, gains = h.get()
            st = TO.step(a["Y_%d" % t], a["iY_%d" % t], a["gains_%d" % t], qref, t, q_rel=max(q_rel, 1e-14))
            ok, skip = TO.compare_state(st, Y, iY, gains)
            assert ok.all(), (t, np.argwhere(~ok)[:5].tolist())
            if (t + 1) % 10 == 0:
                assert abs(cost[0] - a["cost"][(t + 1) // 10 - 1]) <= 1e-9 * abs(cost[0])
            skipped += skip
            total += ok.size
    print("%s: %d of %d entries skipped (sign of dY within the bound)" % (case, skipped, total))
    assert skipped <= max(2, total // 1000)


@pytest.mark.parametrize("case", ["blobs3", "d3", "f2772"])
def test_first_ten_iterations_from_y0(case):
    """run(0, t) from Y0 for t = 1 .. 10 against the oracle's trajectory (from the reference's q), with a tolerance of the summed
    one-step bounds amplified by 4 per step; t = 1, 2 also against the reference's snapshots."""
    g, a = G["cases"][case], A(case)
    Y, iY, gains = a["Y0"], np.zeros_like(a["Y0"]), np.ones_like(a["Y0"])
    q = a["q"]
    tol = np.zeros_like(Y)
    with _handle(a, g) as h:
        for t in range(10):
            st = TO.step(Y, iY, gains, q, t, q_rel=1e-12)
            Y, iY, gains = st.Y, st.iY, st.gains
            tol = 4.0 * tol + st.Y_bound
            h.run(t, t + 1)
            Yg, iYg, gg = h.get()
            assert np.array_equal(gg, gains)
            assert np.all(np.abs(Yg - Y) <= tol), t
            if t + 1 in (1, 2):
                assert np.all(np.abs(Yg - a["Y_%d" % (t + 1)]) <= tol)


# ------------------------------------------------------------------------------------------------ full runs
@pytest.mark.parametrize("case", CASES)
def test_full_run_matches_reference_ensemble(case):
    from frisk_amd.projection import dbscan
    g, a = G["cases"][case], A(case)
    with _handle(a, g) as h:
        cost = h.run(0, 1000)
        Y = h.get()[0]
    assert cost.shape == (100,) and np.isfinite(cost).all()
    assert np.isfinite(Y).all()
    late = cost[10:]                                       # iterations 110 .. 1000: after the exaggeration
    assert late[-1] <= late[0] and np.mean(np.diff(late)) <= 0
    lo, hi = min(g["ensemble_final_cost"]), max(g["ensemble_final_cost"])
    assert 0.9 * lo <= cost[-1] <= 1.1 * hi, (cost[-1], lo, hi)
    labels = dbscan(Y, g["eps"], G["min_samples"])
    assert _same_partition(labels, a["labels"])


def test_runs_are_deterministic_and_resumable():
    g, a = G["cases"]["blobs3"], A("blobs3")
    with _handle(a, g) as h1, _handle(a, g) as h2:
        c1 = h1.run(0, 1000)
        c2 = np.concatenate([h2.run(0, 400), h2.run(400, 1000)])
        s1, s2 = h1.get(), h2.get()
    assert c1.tobytes() == c2.tobytes()
    for x, y in zip(s1, s2):
        assert x.tobytes() == y.tobytes()
    with _handle(a, g) as h3:
        c3 = h3.run(0, 1000)
        assert c3.tobytes() == c1.tobytes() and h3.get()[0].tobytes() == s1[0].tobytes()


def test_tsne_public_function_end_to_end():
    """tsne() from the raw proportions (PCA step on the GPU, Y0 = RandomState(seed).randn) against the reference ensemble."""
    from frisk_amd.projection import dbscan, tsne
    g, a = G["cases"]["blobs3"], A("blobs3")
    r = tsne(a["X"], 2, g["perplexity"], seed=3)
    assert r.Y.shape == (g["n"], 2) and r.cost.shape == (100,) and np.isfinite(r.Y).all()
    assert r.tries.tolist() == a["tries"].tolist()
    assert np.all(np.abs(r.beta - a["beta"]) <= 1e-9 * a["beta"])
    assert _same_partition(dbscan(r.Y, g["eps"], G["min_samples"]), a["labels"])
    small = tsne(a["X"][:7], 3, 2.0)                      # n < 50 is allowed, unlike pca()
    assert small.Y.shape == (7, 3) and np.isfinite(small.Y).all()


# ------------------------------------------------------------------------------------------------ edges against the oracle
def _blobs(n, f, seed):
    rs = np.random.RandomState(seed)
    centres = rs.normal(size=(3, f))
    return centres[rs.randint(0, 3, n)] + 0.3 * rs.normal(size=(n, f))


def _oracle_run(X, Y0, perplexity, iters, h):
    beta, tries, q = TO.affinities(X, perplexity)
    gb, gt, gq = h.affinities(q=True)
    assert gt.tolist() == tries.tolist()
    assert np.all(np.abs(gb - beta) <= 1e-12 * beta)
    assert np.all(np.abs(gq - q) <= TO.q_tolerance(X, beta) * q)
    Y, iY, gains = Y0, np.zeros_like(Y0), np.ones_like(Y0)
    for t in range(iters):
        h.set(Y, iY, gains)
        h.run(t, t + 1)
        st = TO.step(Y, iY, gains, gq, t, gram=False)
        ok, _ = TO.compare_state(st, *h.get())
        assert ok.all(), t
        Y, iY, gains = h.get()


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_row_counts_at_tile_and_block_edges(n):
    from frisk_amd.projection import TSNE
    X = _blobs(n, 5, n)
    Y0 = np.random.RandomState(n + 1).randn(n, 2)
    with TSNE(X, Y0, min(20.0, max(1.5, n / 4.0))) as h:
        _oracle_run(X, Y0, min(20.0, max(1.5, n / 4.0)), 3, h)


@pytest.mark.parametrize("f,d", [(1, 2), (50, 2), (64, 2), (8, 1), (8, 4), (8, 5), (8, 16), (8, 17), (8, 64)])
def test_widths_and_dims(f, d):
    from frisk_amd.projection import TSNE
    n = 130
    X = _blobs(n, f, f * 100 + d)
    Y0 = np.random.RandomState(d).randn(n, d)
    with TSNE(X, Y0, 10.0) as h:
        _oracle_run(X, Y0, 10.0, 3, h)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_sizes_against_oracle(seed):
    from frisk_amd.projection import TSNE
    rs = np.random.RandomState(seed)
    n = int(rs.randint(300, 3001))
    f = int(rs.randint(1, 65))
    X = _blobs(n, f, seed + 7)
    Y0 = rs.randn(n, 2)
    with TSNE(X, Y0, 30.0) as h:
        _oracle_run(X, Y0, 30.0, 5, h)


def test_abi_rejects_bad_input():
    from frisk_amd import _ffi
    L = _ffi.lib()
    E = _ffi.E_ARG
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    X, Y0 = np.random.RandomState(0).rand(20, 4), np.random.RandomState(1).randn(20, 2)
    h = C.c_void_p()
    assert L.frisk_tsne_create(0, p(X), 1, 4, 20.0, 2, p(Y0), C.byref(h)) == E and not h
    assert L.frisk_tsne_create(0, p(X), 50001, 4, 20.0, 2, p(Y0), C.byref(h)) == E and not h
    assert L.frisk_tsne_create(0, p(X), 20, 0, 20.0, 2, p(Y0), C.byref(h)) == E
    X65, Y65 = np.random.RandomState(2).rand(20, 65), np.random.RandomState(3).randn(20, 65)
    assert L.frisk_tsne_create(0, p(X65), 20, 65, 20.0, 2, p(Y0), C.byref(h)) == E
    assert L.frisk_tsne_create(0, p(X), 20, 4, 20.0, 65, p(Y65), C.byref(h)) == E
    assert L.frisk_tsne_create(0, p(X), 20, 4, 20.0, 0, p(Y0), C.byref(h)) == E
    assert L.frisk_tsne_create(0, p(X), 20, 4, 0.0, 2, p(Y0), C.byref(h)) == E
    assert L.frisk_tsne_create(0, p(X), 20, 4, float("nan"), 2, p(Y0), C.byref(h)) == E
    bad = X.copy()
    bad[3, 1] = np.inf
    assert L.frisk_tsne_create(0, p(bad), 20, 4, 20.0, 2, p(Y0), C.byref(h)) == E and not h
    # a row whose sum of exp(-D beta) underflows at every beta tried: the reference's row would be NaN
    far = X.copy() * 1e200
    assert L.frisk_tsne_create(0, p(far), 20, 4, 20.0, 2, p(Y0), C.byref(h)) == _ffi.OK and h
    try:
        beta = np.empty(20)
        assert L.frisk_tsne_affinities(h, p(beta), None, None) == E
        assert L.frisk_tsne_run(h, 0, 10, None) == E
    finally:
        L.frisk_tsne_destroy(h)
    h = C.c_void_p()
    assert L.frisk_tsne_create(0, p(X), 20, 4, 20.0, 2, p(Y0), C.byref(h)) == _ffi.OK
    try:
        assert L.frisk_tsne_run(h, 5, 4, None) == E
        assert L.frisk_tsne_run(h, 0, 1001, None) == E
        nan = np.full_like(Y0, np.nan)
        assert L.frisk_tsne_set(h, p(nan), None, None) == E
        assert L.frisk_tsne_run(h, 0, 10, None) == _ffi.OK
    finally:
        L.frisk_tsne_destroy(h)


# ------------------------------------------------------------------------------------------------ size
def test_twenty_thousand_points_full_run():
    """n = 20 000, f = 50, d = 2, 1000 iterations once: finite, the cost falls after the exaggeration; sampled rows of q
    against the oracle's affinities of those rows."""
    from frisk_amd.projection import TSNE
    n, f = 20000, 50
    X = _blobs(n, f, 11) * 0.2
    Y0 = np.random.RandomState(12).randn(n, 2) * 1e-4
    with TSNE(X, Y0, 30.0) as h:
        beta, tries, q = h.affinities(q=True)
        cost = h.run(0, 1000)
        Y = h.get()[0]
    assert np.isfinite(cost).all() and np.isfinite(Y).all()
    assert cost[-1] < cost[10] and np.mean(np.diff(cost[10:])) < 0
    # sampled rows i: q_ij = max((p_j|i + p_i|j) / 2n, 1e-12 / 4) from the GPU's beta (every conditional row sums to 1)
    rows = np.sort(np.random.RandomState(13).choice(n, 4, replace=False))
    for i in rows:           # beta_i is where the reference's bisection stops: |H - log(perplexity)| <= 1e-5, or 50 tries
        Di = np.delete(((X - X[i]) ** 2).sum(axis=1), i)
        P = np.exp(-Di * beta[i])
        H = np.log(P.sum()) + beta[i] * np.sum(Di * P) / P.sum()
        assert tries[i] == 50 or abs(H - np.log(30.0)) <= 1e-5 * (1 + 1e-6)
    sq = (X * X).sum(axis=1)
    p_col = np.zeros((len(rows), n))           # p_i|j for the sampled i, all j
    for j0 in range(0, n, 2000):
        j1 = min(n, j0 + 2000)
        Dj = np.maximum(sq[j0:j1, None] + sq[None, :] - 2.0 * (X[j0:j1] @ X.T), 0.0)
        E = np.exp(-Dj * beta[j0:j1, None])
        E[np.arange(j1 - j0), np.arange(j0, j1)] = 0.0
        p_col[:, j0:j1] = (E[:, rows] / E.sum(axis=1)[:, None]).T
    for r, i in enumerate(rows):
        E = np.exp(-((X - X[i]) ** 2).sum(axis=1) * beta[i])
        E[i] = 0.0
        want = np.maximum((E / E.sum() + p_col[r]) / (2.0 * n), TO.Q_FLOOR)
        big = want > 1e-6 / n ** 2
        assert np.all(np.abs(q[i] - want)[big] <= 1e-9 * want[big])
        assert np.all(np.abs(q[i] - want) <= 1e-9 * want + 1e-20)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_py_tsne_dbscan_writes_cluster_gff(tmp_path):
    e = G["e2e"]
    out = tmp_path / "T"
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(INPUTS, e["fasta"]), "-t", str(out)] + e["argv"]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "Iteration 1000 : error is" in p.stderr
    assert sorted(os.listdir(out)).count(e["cluster_gff_name"]) == 1
    assert open(out / e["cluster_gff_name"]).read() == e["cluster_gff"]
    assert open(out / "a.gff3").read().splitlines()[0] == e["anomaly_gff"].splitlines()[0]
