"""MDS on the GPU (csrc/mds_kernels.h through frisk_amd.projection.MDS / mds): the dissimilarities and single SMACOF steps against
sklearn's recorded states (tests/golden/mds, tools/make_golden_mds.py) within the forward-error bounds of tests/mds_oracle.py,
full runs against smacof on the same D and against MDS.fit_transform, determinism and resumability, instantiation and tile
edges against the oracle, argument checks of the C ABI, one step at n = 20 000, and the CLI end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mds_oracle as MO
from golden_util import GOLD, INPUTS
from test_mds_cpu import X_of, coincident_X

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "mds.json")))
CASES = sorted(G["cases"])
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def A(case):
    return np.load(os.path.join(GOLD, "mds", G["cases"][case]["file"]))


# ------------------------------------------------------------------------------------------------ dissimilarities
@pytest.mark.parametrize("case", CASES)
def test_dissimilarities_match_exact_and_sklearn(case):
    from frisk_amd.projection import MDS
    g, a = G["cases"][case], A(case)
    X = X_of(case)
    with MDS(X, g["dims"]) as h1, MDS(X, g["dims"]) as h2:
        D, D2 = h1.dissimilarities(), h2.dissimilarities()
    assert D.tobytes() == D2.tobytes()
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0)
    Dx = MO.direct_D(X)
    bound = MO.D_bound_exact(Dx, g["F"])
    assert np.all(np.abs(D - Dx) <= bound)
    rows = a["rows"]
    assert np.all(np.abs(D[rows] - a["Dsk_rows"]) <= bound[rows] + MO.D_bound_gram(X, Dx[rows], rows))
    assert abs(D.sum() - g["D_sum"]) <= 2 * bound.sum()
    if g["dups"]:
        assert np.array_equal(D == 0.0, Dx == 0.0)


# ------------------------------------------------------------------------------------------------ single steps
@pytest.mark.parametrize("case", CASES)
def test_steps_match_sklearn_states(case):
    """for every recorded Y_t of every start: run(Y_t, 1, 0) within the oracle's bound of sklearn's Y_{t+1} and stress_{t+1}"""
    from frisk_amd.projection import MDS
    g, a = G["cases"][case], A(case)
    X = X_of(case)
    worst_y = worst_s = 0.0
    with MDS(X, g["dims"]) as h:
        D = h.dissimilarities()
        dD = MO.D_bound_exact(D, g["F"])
        for k in range(G["n_init"]):
            states, st = a["states_%d" % k], a["stress_%d" % k]
            for t in range(len(st)):
                Y1, s1, it, trace = h.run(states[t], 1, 0.0)
                assert it == 1 and trace.tolist() == [s1]
                b = MO.step_bound(states[t], D, 2 * dD)
                worst_y = max(worst_y, float(np.max(np.abs(Y1 - states[t + 1]) / b)))
                worst_s = max(worst_s, abs(s1 - st[t]) / MO.stress_bound(states[t + 1], D, b))
    print("%s: worst step ratio %.3g, worst stress ratio %.3g" % (case, worst_y, worst_s))
    assert worst_y <= 1.0 and worst_s <= 1.0


def test_step_with_coincident_points():
    from frisk_amd.projection import MDS
    c = G["coincident"]
    a = np.load(os.path.join(GOLD, "mds", c["file"]))
    with MDS(coincident_X(), 2) as h:
        D = h.dissimilarities()
        Y1, s1, _, _ = h.run(a["Y"], 1, 0.0)
    b = MO.step_bound(a["Y"], D, 2 * MO.D_bound_exact(D, 5))
    assert np.all(np.abs(Y1 - a["Y1"]) <= b)
    assert abs(s1 - c["stress1"]) <= MO.stress_bound(a["Y1"], D, b)


# ------------------------------------------------------------------------------------------------ full runs
@pytest.mark.parametrize("case", CASES)
def test_full_run_matches_smacof_and_mds(case):
    from frisk_amd.projection import mds
    g, a = G["cases"][case], A(case)
    r = mds(X_of(case), g["dims"], seed=g["seed"], max_iter=g["max_iter"], eps=g["eps"])
    assert r.n_iters == g["n_iters"]
    floor = 1e-20 * g["D_sum"] ** 2         # stresses at rounding level (n = 2 fits exactly)
    for k in range(G["n_init"]):
        assert abs(r.stresses[k] - g["stresses"][k]) <= 1e-9 * g["stresses"][k] + floor
    if g["n"] == 2:         # every start fits D exactly: which start wins is decided by rounding alone
        assert max(r.stresses) <= floor
        assert abs(np.sqrt(((r.Y[0] - r.Y[1]) ** 2).sum()) - g["D_sum"] / 2) <= 1e-14 * g["D_sum"]
        return
    assert r.best_start == g["best_start"] and r.n_iter == g["n_iter"]
    Ysm = a["states_%d" % g["best_start"]][-1]
    assert np.max(np.abs(r.Y - Ysm)) <= 1e-9 * np.max(np.abs(Ysm))
    assert abs(r.stress - g["stress"]) <= 1e-9 * g["stress"]
    # against MDS.fit_transform (sklearn's Gram-form D)
    assert g["mds_n_iter"] == r.n_iter
    gap = np.max(np.abs(r.Y - a["Y_mds"])) / np.max(np.abs(a["Y_mds"]))
    print("%s: |Y - MDS.fit_transform| / max|Y| = %.2g" % (case, gap))
    assert gap <= 1e-6


def test_runs_are_resumable_and_deterministic():
    from frisk_amd.projection import MDS, mds
    g, a = G["cases"]["blobs44"], A("blobs44")
    X = X_of("blobs44")
    Y0 = a["Y0_0"]
    with MDS(X, 2) as h:
        Y10, s10, n10, tr10 = h.run(Y0, 10, 0.0)
        Y4, _, n4, tr4 = h.run(Y0, 4, 0.0)
        Y6, s6, n6, tr6 = h.run(Y4, 6, 0.0)
    assert (n10, n4, n6) == (10, 4, 6)
    assert Y10.tobytes() == Y6.tobytes() and s10 == s6
    assert np.concatenate([tr4, tr6]).tobytes() == tr10.tobytes()
    r1, r2 = mds(X, 2, seed=g["seed"]), mds(X, 2, seed=g["seed"])
    assert r1.Y.tobytes() == r2.Y.tobytes() and r1.stresses == r2.stresses and r1.n_iters == r2.n_iters
    assert set(r1.timings) == {"dissimilarities_ms", "smacof_ms"}


# ------------------------------------------------------------------------------------------------ edges against the oracle
def _blobs(n, f, seed):
    rs = np.random.RandomState(seed)
    centres = rs.rand(3, f)
    return centres[rs.randint(0, 3, n)] + 0.05 * rs.rand(n, f)


def _oracle_steps(X, d, steps, seed):
    from frisk_amd.projection import MDS
    n, f = X.shape
    Dx = MO.direct_D(X)
    Y = np.random.RandomState(seed).uniform(size=(n, d))
    with MDS(X, d) as h:
        D = h.dissimilarities()
        assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0)
        assert np.all(np.abs(D - Dx) <= MO.D_bound_exact(Dx, f))
        for _ in range(steps):
            Y1, s1, _, _ = h.run(Y, 1, 0.0)
            want = MO.step(Y, D)
            b = MO.step_bound(Y, D)
            assert np.all(np.abs(Y1 - want) <= b)
            assert abs(s1 - MO.stress(want, D)[0]) <= MO.stress_bound(want, D, b)
            Y = Y1


@pytest.mark.parametrize("n", [2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025])
def test_row_counts_at_tile_and_block_edges(n):
    _oracle_steps(_blobs(n, 9, n), 2, 3, n)


@pytest.mark.parametrize("f,d", [(1, 2), (15, 2), (16, 2), (17, 2), (33, 3), (8, 1), (8, 4), (8, 5), (8, 16), (8, 17), (8, 64)])
def test_widths_and_dims(f, d):
    _oracle_steps(_blobs(70, f, 100 * f + d), d, 3, d)


@pytest.mark.parametrize("n,d", [(257, 17), (513, 5), (2049, 2), (2048, 2)])
def test_reductions_past_256_partials(n, d):
    """257, 257, 257 and 256 per-block partials for mds_sum_parts (1, 2 and 8 rows per block): the stress of a sum over more
    than 256 blocks against the oracle's."""
    _oracle_steps(_blobs(n, 9, n + d), d, 3, n)


def test_abi_rejects_bad_input():
    from frisk_amd import _ffi
    L = _ffi.lib()
    E = _ffi.E_ARG
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    X = np.random.RandomState(0).rand(20, 4)
    h = C.c_void_p()
    assert L.frisk_mds_create(0, None, 20, 4, 2, C.byref(h)) == E and not h
    assert L.frisk_mds_create(0, p(X), 20, 4, 2, None) == E
    assert L.frisk_mds_create(0, p(X), 1, 4, 2, C.byref(h)) == E and not h
    assert L.frisk_mds_create(0, p(X), 50001, 4, 2, C.byref(h)) == E and not h
    assert L.frisk_mds_create(0, p(X), 20, 0, 2, C.byref(h)) == E and not h
    assert L.frisk_mds_create(0, p(X), 20, 4, 0, C.byref(h)) == E and not h
    assert L.frisk_mds_create(0, p(X), 20, 4, 65, C.byref(h)) == E and not h
    bad = X.copy()
    bad[3, 1] = np.nan
    assert L.frisk_mds_create(0, p(bad), 20, 4, 2, C.byref(h)) == E and not h
    assert L.frisk_mds_dissimilarities(None, p(np.empty((20, 20)))) == E
    assert L.frisk_mds_create(0, p(X), 20, 4, 2, C.byref(h)) == _ffi.OK and h
    try:
        Y0, Y = np.random.RandomState(1).rand(20, 2), np.empty((20, 2))
        assert L.frisk_mds_dissimilarities(h, None) == E
        assert L.frisk_mds_run(h, p(Y0), 0, 1e-3, p(Y), None, None, None) == E
        assert L.frisk_mds_run(h, p(Y0), 10, -1e-3, p(Y), None, None, None) == E
        assert L.frisk_mds_run(h, p(Y0), 10, float("nan"), p(Y), None, None, None) == E
        assert L.frisk_mds_run(h, p(Y0), 10, 1e-3, None, None, None, None) == E
        inf = Y0.copy()
        inf[0, 0] = np.inf
        assert L.frisk_mds_run(h, p(inf), 10, 1e-3, p(Y), None, None, None) == E
        assert L.frisk_mds_run(h, p(Y0), 10, 1e-3, p(Y), None, None, None) == _ffi.OK
        assert np.isfinite(Y).all()
    finally:
        L.frisk_mds_destroy(h)
    from frisk_amd.projection import mds
    with pytest.raises(ValueError):
        mds(X[:1])


# ------------------------------------------------------------------------------------------------ size
def test_twenty_thousand_points_one_step():
    """n = 20 000, F = 2 772, d = 2: one step against the oracle on 64 fixed rows (their full D rows recomputed in numpy), and
    two runs of 3 steps bit-identical."""
    from frisk_amd.projection import MDS
    n, f = 20000, 2772
    rs = np.random.RandomState(21)
    X = rs.dirichlet(np.full(f, 0.5), size=n)
    Y0 = rs.uniform(size=(n, 2))
    rows = np.sort(np.random.RandomState(22).choice(n, 64, replace=False))
    Dr = MO.direct_D(X, rows)
    with MDS(X, 2) as h:
        Y1, _, _, _ = h.run(Y0, 1, 0.0)
        Ya = h.run(Y0, 3, 0.0)
        Yb = h.run(Y0, 3, 0.0)
    assert Ya[0].tobytes() == Yb[0].tobytes() and Ya[1] == Yb[1]
    diff = Y0[rows][:, None, :] - Y0[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1))
    ratio = Dr / np.where(dist == 0.0, MO.ZERO_DIST, dist)
    ratio[np.arange(64), rows] = 0.0
    want = np.einsum("ij,ijk->ik", ratio, diff) * (1.0 / n)
    norm = np.sqrt((Y0 * Y0).sum(axis=1))
    b = (MO.C_STEP * n * MO.EPS * (ratio * (norm[rows][:, None] + norm[None, :])).sum(axis=1)
         + 2 * MO.D_bound_exact(Dr, f).sum(axis=1)) / n
    assert np.all(np.abs(Y1[rows] - want) <= b[:, None])


# ------------------------------------------------------------------------------------------------ CLI
def _cli(tmp, argv):
    e = G["e2e"]
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(INPUTS, e["fasta"]), "-t", str(tmp)] + argv
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_cli_mds_dbscan_writes_both_gffs(tmp_path):
    e = G["e2e"]
    out = tmp_path / "M"
    p = _cli(out, e["argv"])
    assert "MDS of %d x 44 k-mer proportions" % e["n_anomalous"] in p.stderr
    assert open(out / e["cluster_gff_name"]).read() == e["cluster_gff"]
    got = open(out / "a.gff3").read().splitlines()          # the unmerged anomalous windows (L1672-1675)
    want = e["anomaly_gff"].splitlines()
    assert len(got) == len(want) == e["n_anomalous"] + 1 and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        gf, wf = g.split("\t"), w.split("\t")
        assert gf[:8] == wf[:8]
        gid, gk = gf[8].split(";")
        wid, wk = wf[8].split(";")
        # the window's KLD as the score table prints it (12 significant digits); the reference's value to 1e-11
        assert gid == wid and gk.startswith("KLD=") and abs(float(gk[4:]) - float(wk[4:])) <= 1e-11


def test_cli_mds_kmeans_writes_its_gff(tmp_path):
    e = G["e2e"]
    out = tmp_path / "K"
    argv = e["argv"][:e["argv"].index("--cluster")] + ["--cluster", "KMEANS", "--gffOutfile", "a.gff3"]
    _cli(out, argv)
    text = open(out / e["kmeans_gff_name"]).read()
    assert text.count("\n") == e["n_anomalous"] + text.startswith("##gff-version")
