"""frisk_score_ranges_panel (csrc/panel_kernels.h) on the device: plane p of a panel call against frisk_score_ranges under
profile p, as bytes, at every edge of the profile tile and on both forms; every plane against the reference's scan-loop iteration
(status, nn, GC and RIP exactly, the KLD within kld_oracle_hp.bound(scale), C_KLD = 32); the hand-over between the forms; what the
header promises about reproducibility, the snapshot, the rest of the context and rejected calls.  The ranges are the range set
of tests/ranges_cases.py, the profiles those of tests/panel_cases.py."""
import os

import numpy as np
import pytest

import panel_cases as PC
import ranges_cases as R
from frisk_amd import _ffi
from golden_util import INPUTS

pytestmark = pytest.mark.gpu

TILE = _ffi.PANEL_TILE
COLS = ["status", "kld", "gc", "pi", "si", "cri", "nn"]
SCAN_COLS = ("seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri")


def _engine(kmin, kmax):
    return R.engine(kmin, kmax, prof=None)


def _same(a, b, rip, what=""):
    R.same_columns(a, b, R.score_columns(rip), what=what)


def _singles(e, profs, s, a, b, rip, big=False):
    """score_ranges under each profile in turn; every profile is pushed to the panel on the way."""
    out = []
    for prof in profs:
        PC.install(e, prof)
        out.append(e.score_ranges(s, a, b, rip=rip, big=big))
        assert e.panel_push() == len(out) - 1
    return out


# -------------------------------------------------------------------------------------------- bit identity at the tile edges
@pytest.mark.parametrize("big", [False, True], ids=["auto", "big"])
@pytest.mark.parametrize("kmin,kmax", R.ORDERS)
@pytest.mark.parametrize("P", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_planes_are_the_single_profile_rows(P, kmin, kmax, big):
    rip = kmin <= 2 <= kmax
    s, a, b = R.arrays(R.range_set(kmax))
    with _engine(kmin, kmax) as e:
        single = _singles(e, PC.profiles(P, kmin, kmax), s, a, b, rip, big)
        assert e.panel_size == P
        res = e.score_ranges_panel(s, a, b, rip=rip, big=big)
        assert e.kernel_ms(5) > 0.0
    assert res.status.shape == (P, len(s)) and res.kld.shape == (P, len(s)) and len(res) == len(s)
    for p in range(P):
        _same(res.plane(p), single[p], rip, "plane %d of %d" % (p, P))
    if (kmin, kmax) == (8, 8) and P > 1:
        assert any((res.status[p] != res.status[0]).any() for p in range(1, P))


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("kmin,kmax", [(1, 8), (8, 8), (2, 9)])
def test_every_plane_against_the_oracles(kmin, kmax):
    P = 5
    rows, exp = PC.expected(P, kmin, kmax)
    rip = kmin <= 2 <= kmax
    with _engine(kmin, kmax) as e:
        for prof in PC.profiles(P, kmin, kmax):
            PC.install(e, prof)
            e.panel_push()
        res = e.score_ranges_panel(*R.arrays(rows), rip=rip)
    assert not (res.status & R.JUMPBACK).any()
    for p in range(P):
        R.check("panel k=%d..%d plane %d" % (kmin, kmax, p), res.plane(p), exp[p])


# ------------------------------------------------------------------------------------------------------------ orphan hand-over
def test_handed_over_rows_in_every_plane():
    """The rows of test_orphan_list_hands_over_to_the_long_form: (2, 0, 650) and (2, 0, 65535) overflow the orphan list and
    reach the long form through the device list, with P = TILE + 1 (two tiles)."""
    rows = [(2, 0, 640), (2, 0, 650), (2, 0, 65535), (2, 10, 650), (0, 100, 700)]
    s, a, b = R.arrays(rows)
    P = TILE + 1
    with _engine(1, 8) as e:
        single = _singles(e, PC.profiles(P, 1, 8), s, a, b, True)
        auto = e.score_ranges_panel(s, a, b, rip=True)
        big = e.score_ranges_panel(s, a, b, rip=True, big=True)
    assert (auto.plane(P - 1).status == R.KEPT).all()
    for p in range(P):
        _same(auto.plane(p), single[p], True, "plane %d" % p)
        _same(auto.plane(p), big.plane(p), True, "plane %d, big" % p)


# ------------------------------------------------------------------------------------------------------------ reproducibility
def _take(res, idx):
    from frisk_amd.engine import PanelResult
    cols = {c: getattr(res, c)[idx] for c in ("seq_index", "start", "stop", "gc", "pi", "si", "cri", "nn")}
    return PanelResult(status=np.ascontiguousarray(res.status[:, idx]), kld=np.ascontiguousarray(res.kld[:, idx]), **cols)


def _same_panel(a, b, what=""):
    R.same_columns(a, b, COLS, what=what)


@pytest.mark.parametrize("kmin,kmax", [(1, 8), (2, 9)])
def test_planes_do_not_depend_on_the_call(kmin, kmax):
    import torch
    P = TILE + 1
    profs = PC.profiles(P, kmin, kmax)
    rows = R.range_set(kmax)
    s, a, b = R.arrays(rows)
    n = len(rows)
    with _engine(kmin, kmax) as e:
        for prof in profs:
            PC.install(e, prof)
            e.panel_push()
        first = e.score_ranges_panel(s, a, b, rip=True)
        again = e.score_ranges_panel(s, a, b, rip=True)
        perm = np.random.default_rng(5).permutation(n)
        shuffled = e.score_ranges_panel(s[perm], a[perm], b[perm], rip=True)
        cut = n // 3
        halves = [e.score_ranges_panel(s[:cut], a[:cut], b[:cut], rip=True), e.score_ranges_panel(s[cut:], a[cut:], b[cut:], rip=True)]
        copies = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
        one = rows.index((0, 64, 64 + R.T_SHORT + 1))
        many = e.score_ranges_panel(np.full(copies, s[one]), np.full(copies, a[one]), np.full(copies, b[one]), rip=True)
        # the profiles pushed in another order: the planes are permuted, nothing else changes
        order = np.random.default_rng(6).permutation(P)
        e.panel_reset()
        assert e.panel_size == 0
        for p in order:
            PC.install(e, profs[p])
            e.panel_push()
        reordered = e.score_ranges_panel(s, a, b, rip=True)
    _same_panel(first, again, "again")
    _same_panel(_take(first, perm), shuffled, "permuted")
    _same_panel(_take(first, np.arange(cut)), halves[0], "first part")
    _same_panel(_take(first, np.arange(cut, n)), halves[1], "second part")
    _same_panel(_take(first, np.full(copies, one)), many, "copies")
    for c in ("gc", "pi", "si", "cri", "nn"):
        assert getattr(first, c).tobytes() == getattr(reordered, c).tobytes(), c
    for q, p in enumerate(order):
        assert first.status[p].tobytes() == reordered.status[q].tobytes() and first.kld[p].tobytes() == reordered.kld[q].tobytes(), (q, p)


# ------------------------------------------------------------------------------------------- snapshot and non-interference
def test_the_panel_is_a_copy_and_leaves_the_context_alone():
    kmin, kmax = 1, 8
    A, B = PC.profiles(2, kmin, kmax)
    rows = R.range_set(kmax)
    s, a, b = R.arrays(rows)
    with _engine(kmin, kmax) as e:
        PC.install(e, A)
        rows_a = e.score_ranges(s, a, b, rip=True)
        scan_a = e.scan(5000, 1000, rip=True)
        e.panel_push()
        PC.install(e, B)                                    # the context's profile moves on, the slot does not
        rows_b = e.score_ranges(s, a, b, rip=True)
        res = e.score_ranges_panel(s, a, b, rip=True)
        _same(res.plane(0), rows_a, True, "snapshot")
        assert rows_a.kld.tobytes() != rows_b.kld.tobytes()
        _same(e.score_ranges(s, a, b, rip=True), rows_b, True, "the context's profile after a panel call")
        e.profile_reset()                                   # not even a reset reaches the slot; the panel needs no profile
        _same(e.score_ranges_panel(s, a, b, rip=True).plane(0), rows_a, True, "snapshot after profile_reset")
        PC.install(e, A)
        _same(e.score_ranges(s, a, b, rip=True), rows_a, True, "score_ranges before and after")
        scan_after = e.scan(5000, 1000, rip=True)
        assert len(scan_a) > 0
        for c in SCAN_COLS:
            assert getattr(scan_a, c).tobytes() == getattr(scan_after, c).tobytes(), c
        e.panel_reset()
        assert e.panel_size == 0
        PC.install(e, B)
        assert e.panel_push() == 0
        _same(e.score_ranges_panel(s, a, b, rip=True).plane(0), rows_b, True, "after panel_reset")


# ----------------------------------------------------------------------------------------------------------------- rejections
def test_rejected_panel_calls_launch_nothing():
    from frisk_amd.engine import Engine
    known = [(0, 64, 64 + 513)]
    n0 = len(R.scaffolds()[0])
    prof = R.profile(1, 8)
    exp = R.expect_rows(R.scaffolds(), prof, R._ig(1, 8), known, 1, 8)

    def code(call, *args, **kw):
        with pytest.raises(_ffi.FriskHipError) as err:
            call(*args, **kw)
        return err.value.code

    with Engine(1, 8) as e:
        assert code(e.panel_push) == _ffi.E_STATE                                   # no finalised profile
        assert e.panel_size == 0
        e.load(R.scaffolds())
        assert code(e.score_ranges_panel, *R.arrays(known)) == _ffi.E_STATE         # an empty panel
        PC.install(e, prof)
        assert e.panel_push() == 0
        for bad in ([(4, 0, 10)], [(-1, 0, 10)], [(0, -1, 10)], [(0, 10, 10)], [(0, 10, 9)], [(0, 0, n0 + 1)], [(3, 0, 12)],
                    known + [(0, 5, n0 + 1)]):
            assert code(e.score_ranges_panel, *R.arrays(bad)) == _ffi.E_ARG, bad
            R.check("after a rejected panel call", e.score_ranges_panel(*R.arrays(known), rip=True).plane(0), exp)
        e.load_fasta_shard(os.path.join(INPUTS, "markov_islands.fa"), 400, 150, 0, 1)
        assert code(e.score_ranges_panel, [0], [0], [10]) == _ffi.E_ARG             # a tiled batch
        e.load(R.scaffolds())
        R.check("after a tiled batch", e.score_ranges_panel(*R.arrays(known), rip=True).plane(0), exp)
        # a null required array; n = 0 touches nothing
        s, a, b = R.arrays(known)
        out = np.zeros(1)
        st, nn = np.zeros(1, np.uint32), np.full(1, -7, np.int64)
        p = lambda x: x.ctypes.data_as(__import__("ctypes").c_void_p)               # noqa: E731
        lib = _ffi.lib()
        assert lib.frisk_score_ranges_panel(e._ctx, p(s), p(a), p(b), 1, 0, p(st), None, p(out), None, None, None, p(nn)) == _ffi.E_ARG
        assert lib.frisk_score_ranges_panel(e._ctx, p(s), p(a), p(b), 1, _ffi.SCAN_RIP, p(st), p(out), p(out), None, None, None,
                                            p(nn)) == _ffi.E_ARG
        assert lib.frisk_score_ranges_panel(e._ctx, None, None, None, 0, 0, None, None, None, None, None, None, None) == _ffi.OK
        assert nn[0] == -7
        e.profile_reset()
        assert code(e.panel_push) == _ffi.E_STATE and e.panel_size == 1
    with Engine(3, 5) as e:                                 # a slot is 8 KB here: fill the panel; RIP needs the dinucleotides
        e.load(R.scaffolds())
        PC.install(e, R.profile(3, 5))
        for slot in range(_ffi.PANEL_MAX):
            assert e.panel_push() == slot
        assert code(e.panel_push) == _ffi.E_ARG and e.panel_size == _ffi.PANEL_MAX
        assert code(e.score_ranges_panel, *R.arrays(known), rip=True) == _ffi.E_ARG
        res = e.score_ranges_panel(*R.arrays(known))
        one = e.score_ranges(*R.arrays(known))
        assert res.kld.shape == (_ffi.PANEL_MAX, 1) and (res.kld.view(np.uint64) == one.kld.view(np.uint64)[0]).all()
