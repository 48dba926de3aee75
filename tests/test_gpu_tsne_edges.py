"""Exact t-SNE on the GPU (csrc/tsne_kernels.h through frisk_amd.projection.TSNE) against the extended-precision oracle of
tests/tsne_oracle_hp.py at every launch edge: the cases of tests/tsne_hp_cases.py, each compared as |got - oracle| / unit with the
allowed ratios of tests/golden/tsne_hp.json (8 x what a float64 model reaches on the CPU, tests/test_tsne_hp_cpu.py).  Affinities
at the row-count and width edges of tsne_rows<1> and <8>, on the beta caps, with a large common offset and with one bad row; the
recorded n = 8192 / 8193 cases on either side of tsne_rows<8> / <49>; single steps at every instantiation, row tail, partial
count, phase switch and clamp; and one step whose centring runs past one grid stride."""
import ctypes as C
import os

import numpy as np
import pytest

import tsne_hp_cases as K
import tsne_oracle_hp as HP

pytestmark = pytest.mark.gpu

G = K.golden()
ALLOWED = G["allowed"]
LD = HP.LD


def _y0(n, d=2):
    return np.random.RandomState(n).randn(n, d)


# ------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("cid", [c.id for c in K.AFF])
def test_affinities_against_oracle(cid):
    from frisk_amd.projection import TSNE
    c = K.AFF_BY_ID[cid]
    X = c.X()
    assert K.sha(X) == G["affinity"][cid]["X"]
    o = K.oracle_aff(c)
    with TSNE(X, _y0(c.n), c.perplexity) as h:
        beta, tries, q = h.affinities(q=True)
    r = K.check_aff(c, o, beta, tries, q, ALLOWED["q"])
    print("%s: worst q ratio %.3g (allowed %.3g), tries up to %d" % (cid, r, ALLOWED["q"], tries.max()))


def test_one_bad_row_among_good_ones_is_refused():
    """n = 1025 (tsne_rows<8>), row 1024 at 1e200: its block alone raises the flag; the other 1024 rows alone succeed."""
    from frisk_amd import _ffi
    from frisk_amd.projection import TSNE
    L = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    X, Y0 = K.outlier_X(), _y0(1025)
    h = C.c_void_p()
    assert L.frisk_tsne_create(0, p(X), 1025, 5, 20.0, 2, p(Y0), C.byref(h)) == _ffi.OK and h
    try:
        beta = np.empty(1025)
        assert L.frisk_tsne_affinities(h, p(beta), None, None) == _ffi.E_ARG
        assert L.frisk_tsne_run(h, 0, 1, None) == _ffi.E_ARG
    finally:
        L.frisk_tsne_destroy(h)
    good = np.ascontiguousarray(X[:1024])
    with TSNE(good, Y0[:1024], 20.0) as h2:
        beta, tries = h2.affinities()
        h2.run(0, 1)
        assert np.isfinite(beta).all() and tries.max() < 50 and np.isfinite(h2.get()[0]).all()


@pytest.mark.parametrize("rid", ["n8192_f5", "n8193_f5"])
def test_recorded_affinities_either_side_of_the_register_switch(rid):
    """tsne_rows<8> at n = 8192, tsne_rows<49> at n = 8193 (and tsne_normalise past one grid stride): beta and tries of every row
    equal to the record, six rows of q (own index in register slot 0, 1, 4 and the last) against the record."""
    from frisk_amd.projection import TSNE
    g = G["recorded"][rid]
    n, f, seed = K.RECORDED[rid]
    X = K.blobs(n, f, seed)
    assert K.sha(X) == g["X"]
    beta0, tries0, _mt, _ms = K.recorded_arrays(rid)
    rows = K.SAMPLED_ROWS(n)
    q0 = np.load(os.path.join(K.DIR, rid + "_q.npy")).astype(LD)
    uq = np.load(os.path.join(K.DIR, rid + "_uq.npy")).astype(LD)
    got = []
    for _ in range(2):
        with TSNE(X, _y0(n), g["perplexity"]) as h:
            beta, tries, q = h.affinities(q=True)
        assert np.array_equal(q[rows], q[:, rows].T)
        got.append((beta, tries, q[rows].copy()))
        del q
    beta, tries, qr = got[0]
    assert tries.tolist() == tries0.tolist() and np.array_equal(beta, beta0)
    r = HP.ratio(qr, q0, uq)
    print("%s: worst q ratio on rows %s %.3g (allowed %.3g)" % (rid, rows, r, ALLOWED["q"]))
    assert r <= ALLOWED["q"]
    assert got[1][0].tobytes() == beta.tobytes() and got[1][1].tobytes() == tries.tobytes() and got[1][2].tobytes() == qr.tobytes()


# ------------------------------------------------------------------------------------------------ single steps
@pytest.mark.parametrize("cid", [c.id for c in K.STEPS])
def test_step_against_oracle(cid):
    """set the case's state, run(t, t + 1), get: gains equal, iY, Y and the cost within the allowed ratios."""
    from frisk_amd.projection import TSNE
    c = K.STEP_BY_ID[cid]
    X = c.X()
    o = K.step_aff(c)
    Y, iY, gains = c.state(o["q"])
    g = G["steps"][cid]
    assert [K.sha(a) for a in (X, Y, iY, gains)] == [g[k] for k in ("X", "Y", "iY", "gains")]
    with TSNE(X, Y, c.perplexity) as h:
        beta, tries, q = h.affinities(q=True)
        assert tries.tolist() == o["tries"].tolist() and np.array_equal(beta, o["beta"])
        rq = HP.ratio(q, o["q"], o["u_q"])
        assert rq <= ALLOWED["q"], rq
        q_rel = float(np.max(np.abs(q.astype(LD) - o["q"]) / o["q"]))
        h.set(Y, iY, gains)
        cost = h.run(c.t, c.t + 1)
        Y1, iY1, g1 = h.get()
    st = HP.step(Y, iY, gains, o["q"], c.t, q_rel=q_rel)
    if c.kind == "min_gain":
        assert set(np.unique(st["gains"]).tolist()) == {0.01, 0.0126 * 0.8}
    r = K.check_step(c, st, Y1, iY1, g1, cost, ALLOWED)
    print("%s: worst ratio q %.3g (allowed %.3g), iY %.3g (%.3g), Y %.3g (%.3g), cost %s (%.3g); %d of %d entries skipped" % (
        cid, rq, ALLOWED["q"], r["iY"], ALLOWED["iY"], r["Y"], ALLOWED["Y"], "%.3g" % r["cost"] if "cost" in r else "-",
        ALLOWED["cost"], r["skipped"], Y.size))


# ------------------------------------------------------------------------------------------------ centring past one stride
def test_centring_beyond_one_grid_stride():
    """n = 4097, d = 64: n d = 1024 x 256 + 64, so the last row is centred in the second stride of tsne_centre.  Every beta is
    2^-50 and q = 1 / (n (n - 1)); with D = 0 the unit of q is 16 eps q (g = eps, r = 2 eps, rel_total = 7 eps, + 4 eps)."""
    from frisk_amd.projection import TSNE
    g = G["centring"]
    X, Y0, perplexity = K.centre_inputs()
    n, d = Y0.shape
    assert (K.sha(X), K.sha(Y0)) == (g["X"], g["Y0"]) and n * d > 1024 * 256
    qc = K.centre_q()
    states = []
    for _ in range(2):
        with TSNE(X, Y0, perplexity) as h:
            beta, tries, q = h.affinities(q=True)
            h.run(0, 1)
            states.append((beta, q[K.CENTRE_ROWS].copy()) + h.get())
        off = ~np.eye(n, dtype=bool)
        rq = float(np.max(np.abs(q.astype(LD) - qc)[off] / (16 * HP.EPS * qc)))
        q_rel = float(np.max(np.abs(q.astype(LD) - qc)[off] / qc))
        assert (tries == 50).all() and (beta == 2.0 ** -50).all() and rq <= ALLOWED["q"], rq
        del q
    for a, b in zip(*states):
        assert a.tobytes() == b.tobytes()
    _beta, _q, Y1, iY1, g1 = states[0]
    rows = K.CENTRE_ROWS
    qrows = np.full((len(rows), n), qc, dtype=LD)
    qrows[np.arange(len(rows)), rows] = HP.Q_FLOOR
    st = HP.step(Y0, np.zeros_like(Y0), np.ones_like(Y0), qrows, 0, q_rel=q_rel, rows=rows, S=K.ld(g["S"]), rel_S=K.ld(g["rel_S"]))
    assert set(np.unique(g1).tolist()) <= {0.8, 1.2}
    skip = (g1[rows] != st["gains"]) & K.undecided(st, ALLOWED["dY"])
    assert np.array_equal(g1[rows][~skip], st["gains"][~skip]) and skip.sum() <= K.skip_cap(skip.size)
    r_iY = HP.ratio(iY1[rows], st["iY"], st["u_iY"], ~skip)
    # every entry: Y_new - (Y_old + iY_new) = - the column mean of Y_old + iY_new (the device adds in float64, as here)
    _mean, want, unit = K.centre_unit((Y0 + iY1).astype(LD))
    r_Y = HP.ratio(Y1, want, unit)
    print("centring n%d_d%d: worst ratio q %.3g (allowed %.3g), iY on rows %s %.3g (%.3g), Y - mean on every entry %.3g (%.3g)" % (
        n, d, rq, ALLOWED["q"], rows, r_iY, ALLOWED["iY"], r_Y, g["allowed"]))
    assert r_iY <= ALLOWED["iY"] and r_Y <= g["allowed"]
