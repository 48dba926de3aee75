"""frisk_seq_null (csrc/null_kernels.h) on the device: the bytes of a null batch against frisk_amd/nullmodel.py at every order
form, block edge and table shape; purity in the batch's other sequences, reproducibility, what the call leaves alone and what it
refuses; and the scores of prefix ranges of a null batch on both range forms against the oracles of tests/ranges_cases.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kld_oracle_hp as H
import ranges_cases as R
from golden_util import INPUTS
from oracle import frisk_oracle_np as N

pytestmark = pytest.mark.gpu

# every block edge (the burn-in's 64 steps are no edge of the output, but 63 .. 65 would show a generator that wrote them), an
# empty sequence in the middle, and unequal lengths: sequence index and seq_off differ for every one
LENS = [1, 63, 0, 64, 65, 4095, 4096, 4097, 8193]
SEED = 0x5EEDF00D12345678


@functools.lru_cache(maxsize=None)
def _fixture_profile(kmin, kmax, cut=None):
    seqs = H.read_fasta(os.path.join(INPUTS, "markov_islands.fa"))
    if cut:
        seqs = [seqs[0][:cut]]
    return H.profile(seqs, kmin, kmax)


@functools.lru_cache(maxsize=None)
def _big_profile():
    """kmin..kmax = 1..3 with counts of up to 2^61 in the table the order-2 chain reads (and one empty context)."""
    from frisk_amd.engine import profile_len, table_offset
    rng = np.random.default_rng(11)
    sym = rng.integers(1, 1000, profile_len(1, 3)).astype(np.int64)
    tab = rng.integers(1, 1 << 61, 64).astype(np.int64)
    tab[20:24] = [(1 << 62) - 1, 1, 0, (1 << 33) + 5]
    tab[40:44] = 0
    sym[table_offset(1, 3):] = tab
    return sym, (1000, 0, 0)


@functools.lru_cache(maxsize=None)
def _want(kmin, kmax, order, which):
    from frisk_amd import nullmodel as M
    sym, meta = _profile(kmin, kmax, which)
    return M.generate_batch(sym, kmin, order, SEED, LENS)


def _profile(kmin, kmax, which):
    if which == "big":
        return _big_profile()
    return _fixture_profile(kmin, kmax, 200 if which == "host200" else None)


def _engine(kmin, kmax, prof):
    return R.engine(kmin, kmax, seqs=None, prof=prof)


def _batch(e):
    return [e.read_seq(i) for i in range(e.n_seq)]


# ------------------------------------------------------------------------------------------------------------------- bytes
@pytest.mark.parametrize("kmin,kmax,order,which", [(1, 8, 0, "fixture"), (1, 8, 1, "fixture"), (1, 8, 3, "fixture"), (1, 8, 7, "fixture"),
                                                   (3, 5, 2, "fixture"), (3, 5, 4, "fixture"), (8, 8, 7, "fixture"),
                                                   (1, 8, 3, "host200"), (1, 3, 2, "big")])
def test_bytes_equal_the_numpy_generator(kmin, kmax, order, which):
    """host200: the profile of a 200-base host, where most order-3 contexts are empty; big: counts above 2^32."""
    want = _want(kmin, kmax, order, which)
    with _engine(kmin, kmax, _profile(kmin, kmax, which)) as e:
        assert e.kernel_ms(6) < 0
        e.null_batch(LENS, SEED, order)
        assert e.n_seq == len(LENS) and e.seq_lens == LENS and e.kernel_ms(6) > 0.0
        got = _batch(e)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, LENS[i], next(j for j in range(len(w)) if g[j] != w[j]))
    assert set(b"".join(want)) <= set(b"ATGC")


def test_purity_and_reproducibility():
    with _engine(1, 8, _fixture_profile(1, 8)) as e:
        e.null_batch([10, 5000], 42, 5)
        first = _batch(e)
        e.null_batch([77, 5000], 42, 5)
        other = _batch(e)
        e.null_batch([10, 5000], 42, 5)
        again = _batch(e)
        e.null_batch([10, 5000], 43, 5)
        seeded = _batch(e)
        e.null_batch([], 42, 5)
        assert e.n_seq == 0
        e.null_batch([0, 0], 42, 5)
        assert _batch(e) == [b"", b""]
    assert first[1] == other[1] and other[0][:10] == first[0] and len(other[0]) == 77      # purity: the batch's shape does not enter
    assert again == first and seeded[1] != first[1] and seeded[0] != first[0]


# ------------------------------------------------------------------------------------------------------------------- state
_same = R.same_columns


def test_the_call_leaves_profile_panel_and_rows_alone():
    from frisk_amd.engine import Engine
    rows = [(0, 64, 700), (1, 0, 65536), (1, 29000, 43000), (2, 0, 650), (0, 0, 77)]
    cols = ["status", "nn", "kld", "gc", "pi", "si", "cri"]
    sym, meta = R.profile(1, 8)
    with Engine(1, 8) as e:
        e.load(R.scaffolds())
        fx = _fixture_profile(1, 8)
        e.profile_set(fx[0], *[int(v) for v in fx[1]])
        e.panel_push()
        e.profile_set(sym, *[int(v) for v in meta])
        e.panel_push()
        before = (e.score_ranges(*R.arrays(rows), rip=True), e.score_ranges_panel(*R.arrays(rows), rip=True), e.scan(5000, 1000, rip=True))
        prof = e.profile_get()
        e.null_batch([300, 9000, 5], 7, 7)
        assert e.seq_lens == [300, 9000, 5] and e.panel_size == 2
        now = e.profile_get()
        assert now[0].tobytes() == prof[0].tobytes() and now[1:] == prof[1:]
        plan = e.scan_plan(200, 100)                                    # the plan follows the new batch
        assert plan == len([1 for n in (300, 9000, 5) for _ in N.iter_windows(n, 200, 100, False)])
        e.load(R.scaffolds())
        after = (e.score_ranges(*R.arrays(rows), rip=True), e.score_ranges_panel(*R.arrays(rows), rip=True), e.scan(5000, 1000, rip=True))
    assert len(before[2]) > 0
    assert _same(before[0], after[0], cols) and _same(before[1], after[1], cols)
    assert _same(before[2], after[2], ["seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri"])


def test_a_staged_batch_survives_the_call():
    """As with frisk_seq_synth2: the null batch takes the resident slot, the staged one still commits."""
    from frisk_amd import nullmodel as M
    fx = _fixture_profile(1, 8)
    staged = [R.scaffolds()[0], R.scaffolds()[3]]
    with _engine(1, 8, fx) as e:
        e.load([b"ACGT" * 10])
        e.stage(staged)
        e.null_batch([100, 4100], 1, 3)
        assert _batch(e) == M.generate_batch(fx[0], 1, 3, 1, [100, 4100])
        e.commit()
        got = _batch(e)
    want = [bytes(bytearray(c if c in b"ACGTacgt" else ord("N") for c in s)) for s in staged]
    assert got == want


def test_refused_calls_launch_nothing_and_keep_the_batch():
    from frisk_amd import _ffi
    from frisk_amd.engine import Engine

    def code(e, lens, order):
        with pytest.raises(_ffi.FriskHipError) as err:
            e.null_batch(lens, 1, order)
        return err.value.code

    with Engine(1, 8) as e:
        assert code(e, [10], 3) == _ffi.E_STATE                         # no profile at all
        e.load([b"ACGTTGCA" * 40])
        e.profile_reset(); e.profile_add()
        assert code(e, [10], 3) == _ffi.E_STATE                         # not finalised
        e.profile_finalize()
        kept = _batch(e)
        for lens, order in (([10], -1), ([10], 8), ([10, -1], 3), ([-5], 0)):
            assert code(e, lens, order) == _ffi.E_ARG, (lens, order)
            assert e.kernel_ms(6) < 0 and _batch(e) == kept
        lib = _ffi.lib()
        assert lib.frisk_seq_null(e._ctx, None, 1, 1, 3) == _ffi.E_ARG
        one = (C.c_int64 * 1)(10)
        assert lib.frisk_seq_null(e._ctx, one, -1, 1, 3) == _ffi.E_ARG
        assert _batch(e) == kept
        e.null_batch([10], 1, 7)
        assert len(e.read_seq(0)) == 10
        e.profile_reset()
        assert code(e, [10], 3) == _ffi.E_STATE
    with Engine(3, 5) as e:
        fx = _fixture_profile(3, 5)
        e.profile_set(fx[0], *[int(v) for v in fx[1]])
        assert code(e, [10], 1) == _ffi.E_ARG and code(e, [10], 5) == _ffi.E_ARG      # order + 1 < kmin, > kmax
        e.null_batch([10], 1, 2)
        e.null_batch([10], 1, 4)


# ------------------------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("kmin,kmax,order", [(1, 8, 7), (3, 5, 4)])
def test_prefix_ranges_of_a_null_batch_against_the_oracles(kmin, kmax, order):
    """Lengths around kmax, a block and FRISK_RANGE_SHORT_MAX (65 535 | 65 536: the short and the long form), of each of three
    sequences, scored on the device batch and - by the oracles - on the numpy generator's bytes."""
    from frisk_amd import nullmodel as M
    prof = R.profile(kmin, kmax)
    lengths = [7, 8, 64, 4096, 4097, 5000, 65535, 65536]
    rows = [(s, 0, n) for s in range(3) for n in lengths]
    seqs = M.generate_batch(prof[0], kmin, order, 99, [65536] * 3)
    exp = R.expect_rows(seqs, prof, R._ig(kmin, kmax), rows, kmin, kmax)
    assert all(x["nn"] == 0 and x["status"] & R.KEPT for x in exp)
    assert sum(x["flag"] == H.OK for x in exp) >= 18
    with _engine(kmin, kmax, prof) as e:
        e.null_batch([65536] * 3, 99, order)
        res = e.score_ranges(*R.arrays(rows), rip=kmin <= 2 <= kmax)
    assert not res.nn.any()
    R.check("null prefixes k=%d..%d order %d" % (kmin, kmax, order), res, exp)
