"""IncrementalPCA on the GPU per entry (frisk_ipca_* of csrc/ipca_kernels.h through the C ABI and frisk_amd.projection.IncrementalPCA)
against the long-double oracle of tests/ipca_oracle_hp.py, at the shapes and inputs of tests/ipca_hp_cases.py.

What is compared is what the device computes: the Gram matrix G that frisk_ipca_gram returns (never compared before), the mean and
variance that a commit installs, and Y of a transform - each entry against the oracle in units of its own forward error, with the
tolerance of tests/golden/ipca_hp.json (8 x the worst ratio of the float64 restatement on the same cases; nothing in it was measured
on a device).  Then the transform's rows and piece boundaries, the independence of every result from what the handle did before
(bit for bit), and the pending-batch state.  Every test prints its worst ratio before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import ipca_hp_cases as K
import ipca_oracle_hp as HP

pytestmark = pytest.mark.gpu

TOL = K.golden()["tolerance"]
PIECE = (1 << 23) // 2816           # rows per transform piece at f = 2772 (f_pad 2816)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _gram(fit, Xb):
    from frisk_amd import _ffi
    Xb = np.ascontiguousarray(Xb, dtype=np.float64)
    G = np.full((fit.f, fit.f), np.nan)
    assert _ffi.lib().frisk_ipca_gram(fit._h, _p(Xb), Xb.shape[0], _p(G)) == _ffi.OK
    return G


def _commit(fit, S, Vt):
    from frisk_amd import _ffi
    S, Vt = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(Vt, dtype=np.float64)
    return _ffi.lib().frisk_ipca_commit(fit._h, _p(S), _p(Vt))


def _install(fit, i):
    if i.state is None:
        fit.set_state(0)
    else:
        fit.set_state(i.state["n"], i.state["mean"], i.state["var"], i.state["S"], i.state["Vt"])


def _run(fit, cid, between=None):
    """The case on this handle: its state installed, gram, (between), commit, get, transform.  {G, mean, var, Y}."""
    from frisk_amd import _ffi
    c, i = K.BY_ID[cid], K.inputs(cid)
    _install(fit, i)
    G = _gram(fit, i.Xb)
    if between:
        between(fit)
    assert _commit(fit, i.S_new, i.Vt_new) == _ffi.OK
    n, mean, var, S, Vt = fit.state()
    assert n == c.seen + c.b and S.tobytes() == i.S_new.tobytes() and Vt.tobytes() == i.Vt_new.tobytes()
    return {"G": G, "mean": mean, "var": var, "Y": fit.transform(K.transform_rows(cid))}


def _same(a, b):
    return all(a[q].tobytes() == b[q].tobytes() for q in K.QUANTITIES)


# ------------------------------------------------------------------------------------------------ per case
@pytest.mark.parametrize("cid", [c.id for c in K.CASES])
def test_gram_statistics_and_transform_per_entry(cid):
    from frisk_amd.projection import IncrementalPCA
    c = K.BY_ID[cid]
    with IncrementalPCA(c.f, c.d) as fit:
        got = _run(fit, cid)
    r = K.compare(cid, got)
    print("%s: worst |GPU - oracle| / unit: %s (tolerance %s)" % (cid, {q: "%.3g" % v for q, v in r.items()},
                                                                   {q: "%.3g" % v for q, v in TOL.items()}))
    assert np.array_equal(got["G"], got["G"].T)
    assert set(r) == set(K.QUANTITIES)
    K.check(cid, got, TOL, what="GPU")


# ------------------------------------------------------------------------------------------------ transform rows
STATE9 = "later_rows/b13_f9_d2_seen7/kmer"


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_transform_of_one_to_five_rows(m):
    """proj_transform takes four rows per block: a last block of 1, 2, 3 rows, one block exactly, and one row past it."""
    from frisk_amd.projection import IncrementalPCA
    i = K.inputs(STATE9)
    X = K.transform_rows(STATE9)
    with IncrementalPCA(9, 2) as fit:
        _install(fit, i)
        Y, Yall = fit.transform(X[:m]), fit.transform(X)
    want, unit = HP.transform(X[:m], i.state["mean"], i.state["Vt"])
    r = HP.ratio(Y, want, unit)
    print("transform of %d rows, f = 9: worst |GPU - oracle| / unit %.3g (tolerance %.3g)" % (m, r, TOL["Y"]))
    assert Y.shape == (m, 2) and Y.tobytes() == Yall[:m].tobytes()
    assert r <= TOL["Y"]


@functools.lru_cache(maxsize=None)
def _wide():
    """5957 = 2 PIECE + 1 rows of 2772 k-mer proportions and a mean to centre them with."""
    rs = np.random.RandomState(2772)
    centres = K._blobs(rs, 2772)
    X = K._draw(rs, centres, rs.randint(0, 3, 2 * PIECE + 1), 2772)
    return X, X[:100].mean(axis=0)


def _sample_rows(n):
    """200 rows of n: the first, the last, two on each side of every piece boundary below n, and seeded rows of the first piece."""
    edge = [r for k in (1, 2) for r in (k * PIECE - 2, k * PIECE - 1, k * PIECE, k * PIECE + 1) if 0 <= r < n]
    fixed = sorted(set([0, n - 1] + edge))
    pool = [r for r in np.random.RandomState(7).permutation(PIECE - 3).tolist() if r not in fixed]
    return np.array(sorted(fixed + pool[:200 - len(fixed)]), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _wide_oracle(d):
    """(Vt, {row: (Y, unit)}) for every row any _sample_rows(n) can name: computed once per d."""
    X, mean = _wide()
    Vt = K._orthonormal(np.random.RandomState(100 + d), d, 2772)
    rows = sorted(set(np.concatenate([_sample_rows(n) for n in (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 1)]).tolist()))
    Y, unit = HP.transform(X[rows], mean, Vt)
    return Vt, {r: (Y[k], unit[k]) for k, r in enumerate(rows)}


@pytest.mark.parametrize("d", [1, 2, 64])
@pytest.mark.parametrize("n", [PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 1])
def test_transform_across_piece_boundaries(n, d):
    from frisk_amd.projection import IncrementalPCA
    assert PIECE == 2978
    X, mean = _wide()
    Vt, table = _wide_oracle(d)
    rows = _sample_rows(n)
    assert len(rows) == 200 and (n <= PIECE or {PIECE - 1, PIECE} <= set(rows.tolist()))
    with IncrementalPCA(2772, d) as fit:
        fit.set_state(1000, mean, np.ones(2772), np.linspace(2.0, 1.0, d), Vt)
        Y = fit.transform(X[:n])
        single = np.vstack([fit.transform(X[r:r + 1]) for r in rows])
    want = np.vstack([table[r][0] for r in rows])
    unit = np.vstack([table[r][1] for r in rows])
    r = HP.ratio(Y[rows], want, unit)
    print("transform of %d x 2772, d = %d: worst |GPU - oracle| / unit on 200 rows %.3g (tolerance %.3g)" % (n, d, r, TOL["Y"]))
    assert Y.shape == (n, d) and np.isfinite(Y).all()
    assert Y[rows].tobytes() == single.tobytes()            # a row's result does not depend on the piece or block it falls in
    assert r <= TOL["Y"]


# ------------------------------------------------------------------------------------------------ history
def _use(fit, b):
    """Work that grows every buffer of the handle past what a batch of b rows needs: a larger batch, a transform of more rows, a
    smaller batch."""
    from frisk_amd import _ffi
    rs = np.random.RandomState(b)
    S, Vt = np.linspace(3.0, 1.0, fit.dims), K._orthonormal(rs, fit.dims, fit.f)
    fit.set_state(0)
    _gram(fit, rs.rand(3 * b + 50, fit.f))
    assert _commit(fit, S, Vt) == _ffi.OK
    fit.transform(rs.rand(5 * b + 100, fit.f))
    _gram(fit, rs.rand(2, fit.f))
    assert _commit(fit, S, Vt) == _ffi.OK


HISTORY = ["later_rows/b29_f9_d2_seen7/unperm", "first_b/b17_f9_d2/offset", "first_b/b129_f9_d2/kmer",
           "later_f257/b40_f257_d2_seen100000/zeroconst", "first_f/b40_f257_d2/kmer", "later_d/b20_f70_d64_seen1/sspan"]


@pytest.mark.parametrize("cid", HISTORY)
def test_results_do_not_depend_on_the_handles_history(cid):
    from frisk_amd.projection import IncrementalPCA
    c, i = K.BY_ID[cid], K.inputs(cid)
    with IncrementalPCA(c.f, c.d) as fresh, IncrementalPCA(c.f, c.d) as used, IncrementalPCA(c.f, c.d) as twice:
        want = _run(fresh, cid)
        _use(used, c.b)
        got = _run(used, cid)
        assert _same(got, want), "a handle that has grown its buffers computes other bits"
        again = _run(used, cid)
        assert _same(again, want)
        # gram twice before the commit: the second one wins
        _install(twice, i)
        other = np.random.RandomState(5).rand(c.b + 7, c.f)
        _gram(twice, other)
        got2 = _run(twice, cid, between=None)
        assert _same(got2, want)
        _install(twice, i)
        G1 = _gram(twice, other)
        G2 = _gram(twice, i.Xb)
        from frisk_amd import _ffi
        assert _commit(twice, i.S_new, i.Vt_new) == _ffi.OK
        n, mean, var, _S, _Vt = twice.state()
        assert n == c.seen + c.b and G2.tobytes() == want["G"].tobytes() and G1.tobytes() != G2.tobytes()
        assert mean.tobytes() == want["mean"].tobytes() and var.tobytes() == want["var"].tobytes()
        assert twice.transform(K.transform_rows(cid)).tobytes() == want["Y"].tobytes()
    r = K.check(cid, want, TOL, what="GPU")
    print("%s: fresh, used and gram-twice handles agree bit for bit; worst ratio %s" % (cid, {q: "%.3g" % v for q, v in r.items()}))


# ------------------------------------------------------------------------------------------------ pending batch
def test_gram_alone_leaves_the_state_unchanged():
    from frisk_amd.projection import IncrementalPCA
    cid = "later_rows/b14_f9_d2_seen100000/unperm"
    i = K.inputs(cid)
    with IncrementalPCA(9, 2) as fit:
        _install(fit, i)
        before = fit.state()
        Ybefore = fit.transform(i.foreign)
        _gram(fit, i.Xb)
        after = fit.state()
        assert before[0] == after[0] == i.state["n"]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[1:], after[1:]))
        assert all(a.tobytes() == np.asarray(i.state[k]).tobytes() for a, k in zip(after[1:], ("mean", "var", "S", "Vt")))
        assert fit.transform(i.foreign).tobytes() == Ybefore.tobytes()


@pytest.mark.parametrize("cid", ["later_rows/b14_f9_d2_seen7/kmer", "first_b/b65_f9_d2/zeroconst"])
def test_transform_between_gram_and_commit_does_not_change_the_commit(cid):
    from frisk_amd.projection import IncrementalPCA
    c, i = K.BY_ID[cid], K.inputs(cid)
    many = np.random.RandomState(3).rand(4 * c.b + 33, c.f)

    def between(fit):
        if c.seen:                                  # (an unfitted handle has nothing to transform with)
            fit.transform(many)
    with IncrementalPCA(c.f, c.d) as plain, IncrementalPCA(c.f, c.d) as busy:
        want = _run(plain, cid)
        if not c.seen:                              # a first batch: fit something, then the case as a later batch on both handles
            for fit in (plain, busy):
                _use(fit, 5)
            n, mean, var, S, Vt = plain.state()
            for fit in (plain, busy):
                fit.set_state(n, mean, var, S, Vt)
            Gp, Gb = _gram(plain, i.Xb), _gram(busy, i.Xb)
            busy.transform(many)
            from frisk_amd import _ffi
            assert _commit(plain, i.S_new, i.Vt_new) == _ffi.OK and _commit(busy, i.S_new, i.Vt_new) == _ffi.OK
            assert Gp.tobytes() == Gb.tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plain.state()[1:], busy.state()[1:]))
            assert plain.state()[0] == busy.state()[0] == n + c.b
        else:
            got = _run(busy, cid, between=between)
            assert _same(got, want)
    K.check(cid, want, TOL, what="GPU")


def test_set_drops_a_pending_batch():
    from frisk_amd import _ffi
    from frisk_amd.projection import IncrementalPCA
    cid = "later_rows/b13_f9_d2_seen1/kmer"
    i = K.inputs(cid)
    with IncrementalPCA(9, 2) as fit:
        _install(fit, i)
        _gram(fit, i.Xb)
        _install(fit, i)
        assert _commit(fit, i.S_new, i.Vt_new) == _ffi.E_STATE
        assert fit.state()[0] == 1 and fit.state()[1].tobytes() == i.state["mean"].tobytes()
        _gram(fit, i.Xb)
        fit.set_state(0)
        assert _commit(fit, i.S_new, i.Vt_new) == _ffi.E_STATE
        assert fit.state()[0] == 0
        _gram(fit, i.Xb)
        assert _commit(fit, i.S_new, i.Vt_new) == _ffi.OK and fit.state()[0] == 13
