"""frisk_window_vectors (csrc/kvec_kernels.h) against the numpy oracle, bit for bit: the values are integer counts and one
correctly rounded division, so every comparison is == on .tolist().  The oracle of a range is the oracle of its SLICE: a word
that reaches past the range's end, or a fetch that is off by a base, changes a count."""
import json
import os

import numpy as np
import pytest

from golden_util import GOLD

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "projection_counts.json")))
ORDERS = [(1, 1), (1, 6), (3, 5), (6, 6), (7, 7), (1, 7)]


def want(seq, a, b):
    from frisk_amd.projection import proportions_from_forward
    from oracle import frisk_oracle_np as N
    return proportions_from_forward(N.forward_counts(N.Encoded(seq), a, b)[0], a, b).tolist()


def want_nn(seq):
    return sum(ch not in "ATGC" for ch in seq)


def width(a, b):
    from frisk_amd.projection import feature_keys
    return len(feature_keys(a, b))


@pytest.fixture(scope="module")
def eng():
    from frisk_amd import Engine
    with Engine(1, 2) as e:             # the context's own orders play no part
        yield e


def check(e, seqs, ranges, a, b, batch_rows=0):
    """ranges (scaffold, start, stop) of the loaded `seqs`: rows, nn and status against the oracle of each slice."""
    X, nn, st = e.window_vectors([r[0] for r in ranges], [r[1] for r in ranges], [r[2] for r in ranges], a, b, batch_rows)
    assert X.shape == (len(ranges), width(a, b))
    for row, got_nn, got_st, (s, lo, hi) in zip(X, nn.tolist(), st.tolist(), ranges):
        assert row.tolist() == want(seqs[s][lo:hi], a, b), (s, lo, hi, a, b)
        assert got_nn == want_nn(seqs[s][lo:hi]) and got_st == 0, (s, lo, hi, got_nn, got_st)
    return X


def test_golden_windows_as_whole_scaffolds(eng):
    seqs = [w["seq"] for w in G["windows"]]
    eng.load(seqs)
    X, nn, st = eng.window_vectors(range(len(seqs)), [0] * len(seqs), [len(s) for s in seqs], G["pcaMin"], G["pcaMax"])
    for row, w in zip(X, G["windows"]):
        assert row.tolist() == w["vector"]
    assert nn.tolist() == [want_nn(s) for s in seqs] and not st.any()
    assert eng.kernel_ms(3) > 0.0


def test_golden_windows_embedded_between_valid_flanks(eng):
    """Every window at an offset that is no multiple of the 16 bases of a code word, valid bases of the same scaffold on both
    sides: a word that crosses the range's end is counted from real bases and shows."""
    rng = np.random.default_rng(21)
    wins = [w for i in range(7) for w in [G["windows"][i % len(G["windows"])]]]
    parts, ranges, pos = [], [], 0
    for flank, w in zip((1, 15, 16, 17, 31, 32, 33), wins):
        parts.append("".join(rng.choice(list("ACGT"), size=flank)))
        pos += flank
        ranges.append((0, pos, pos + len(w["seq"])))
        parts.append(w["seq"])
        pos += len(w["seq"])
    parts.append("".join(rng.choice(list("ACGT"), size=33)))
    scaffold = "".join(parts)
    eng.load([scaffold])
    X, _nn, st = eng.window_vectors([0] * 7, [r[1] for r in ranges], [r[2] for r in ranges], G["pcaMin"], G["pcaMax"])
    for row, w in zip(X, wins):
        assert row.tolist() == w["vector"]
    assert not st.any()


def edge_scaffold():
    rng = np.random.default_rng(33)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))          # noqa: E731
    # 0..1500 bases, 1500..1540 N, 1540..2540 bases, 2540..2840 lowercase, 2840..4040 bases
    return rand(1500) + "N" * 40 + rand(1000) + rand(300).lower() + rand(1200)


@pytest.mark.parametrize("a,b", ORDERS)
def test_range_edges(eng, a, b):
    from frisk_amd import _ffi
    s = edge_scaffold()
    wg = _ffi.KVEC_THREADS
    ranges = [(0, 64 + r, 64 + r + n) for r in (0, 1, 15, 16, 17, 31) for n in (b, b + 1, 31, 32, 33, 63, 64, 65, wg - 1, wg, wg + 1)]
    ranges += [(0, len(s) - 100, len(s)),       # ends on the scaffold's last base: the next position is PAD
               (0, 0, 77),                      # starts at 0
               (0, 1400, 1500),                 # the next base is N
               (0, 1540, 1640),                 # the previous base is N
               (0, 1380, 1700),                 # the N run inside
               (0, 2400, 3000),                 # the lowercase run inside
               (0, 0, len(s))]
    eng.load([s])
    check(eng, [s], ranges, a, b)
    # all lowercase: the vector of the uppercase text, every base unresolved for the 30 % rule
    X, nn, st = eng.window_vectors([0], [2540], [2840], a, b)
    assert X[0].tolist() == want(s[2540:2840].upper(), a, b) and nn.tolist() == [300] and st.tolist() == [0]


def test_palindromes_and_counters_past_sixteen_bits(eng):
    seqs = ["AT" * 40, "A" * 70000]
    eng.load(seqs)
    check(eng, seqs, [(0, 0, 80), (1, 0, 70000), (0, 1, 80), (1, 3, 69999)], 1, 6)
    X = check(eng, seqs, [(0, 0, 80)], 2, 2)
    assert X[0].tolist().count(0.0) == 8 and sorted(set(X[0].tolist()))[1:] == [78.0 / 158.0, 80.0 / 158.0]     # 39 TA and 40 AT, each its own mirror: twice


def test_status_names_the_orders_without_a_word(eng):
    from frisk_amd import _ffi
    rng = np.random.default_rng(5)
    s = "".join(rng.choice(list("ACGT"), size=40)) + "AC" + "N" + "GTA" + "CCGT"
    eng.load([s])
    a, b = 1, 5
    bit = lambda x: 1 << (_ffi.KVEC_ORDER_SHIFT + x)                    # noqa: E731
    X, nn, st = eng.window_vectors([0, 0, 0], [7, 40, 3], [7 + b - 1, 46, 3 + b], a, b)
    # b - 1 bases: no word of order b; the shorter orders are exact
    assert st[0] == (_ffi.KVEC_EMPTY_ORDER | bit(5)) and X[0, :width(1, 4)].tolist() == want(s[7:11], 1, 4)
    # b valid bases with an N in the middle (AC N GTA): the longest run is 3
    assert st[1] == (_ffi.KVEC_EMPTY_ORDER | bit(4) | bit(5)) and X[1, :width(1, 3)].tolist() == want(s[40:46], 1, 3)
    assert nn.tolist() == [0, 1, 0]
    assert st[2] == 0 and X[2].tolist() == want(s[3:8], a, b)             # exactly b bases: one word of order b
    assert np.isfinite(X).all()


def test_launch_shapes(eng):
    from frisk_amd import _ffi
    s = edge_scaffold()
    eng.load([s])
    X, nn, st = eng.window_vectors([], [], [], 1, 6)
    assert X.shape == (0, 2772) and nn.shape == (0,) and st.shape == (0,)
    check(eng, [s], [(0, 5, 405)], 1, 6)
    # more ranges than workgroups: the grid-stride loop, and the counters cleared between a workgroup's ranges
    n = _ffi.KVEC_GRID_CAP + 1
    starts = [(37 * i) % 1400 for i in range(n)]
    X, nn, st = eng.window_vectors([0] * n, starts, [p + 16 for p in starts], 1, 3)
    rows = {p: want(s[p:p + 16], 1, 3) for p in set(starts)}
    assert X.tolist() == [rows[p] for p in starts] and not nn.any() and not st.any()
    # batches of rows, a permutation of the rows, and the same call twice
    ranges = [(0, 3, 300), (0, 1450, 1600), (0, 17, 4000), (0, 2500, 2900), (0, 31, 63), (0, 1000, 1257), (0, 4000, 4040)]
    whole = check(eng, [s], ranges, 1, 6)
    assert check(eng, [s], ranges, 1, 6, batch_rows=3).tolist() == whole.tolist()
    assert check(eng, [s], ranges, 1, 6, batch_rows=1).tolist() == whole.tolist()
    perm = [4, 0, 6, 2, 5, 1, 3]
    assert check(eng, [s], [ranges[i] for i in perm], 1, 6, batch_rows=2).tolist() == whole[perm].tolist()
    assert check(eng, [s], ranges, 1, 6).tobytes() == whole.tobytes()


def rejected(e, *args):
    from frisk_amd import _ffi
    with pytest.raises(_ffi.FriskHipError) as err:
        e.window_vectors(*args)
    return err.value.code == _ffi.E_ARG


def test_rejections_return_e_arg(eng):
    from frisk_amd import Engine
    s = edge_scaffold()
    with Engine(1, 4) as fresh:
        assert rejected(fresh, [0], [0], [10], 1, 3)                    # no resident batch
        fasta = os.path.join(GOLD, "inputs", "markov_islands.fa")
        fresh.load_fasta_shard(fasta, 400, 150, 0, 1)
        assert rejected(fresh, [0], [0], [10], 1, 3)                    # a tiled batch
    eng.load([s, s[:100]])
    for args in (([2], [0], [10], 1, 3), ([-1], [0], [10], 1, 3),       # an index out of range
                 ([0], [-1], [10], 1, 3),                               # start < 0
                 ([0], [10], [10], 1, 3), ([0], [11], [10], 1, 3),      # stop <= start
                 ([1], [0], [101], 1, 3), ([0, 1], [0, 90], [10, 4000], 1, 3),   # stop > seq_len (of THAT scaffold)
                 ([0], [0], [10], 0, 3), ([0], [0], [10], 3, 2), ([0], [0], [10], 1, 8), ([0], [0], [10], 8, 8)):
        assert rejected(eng, *args), args
    check(eng, [s, s[:100]], [(1, 0, 100), (0, 90, 4000)], 1, 3)        # the batch is as it was


def test_window_vectors_route_equals_symmetric_counts(eng):
    from frisk_amd.projection import symmetricCounts, windowVectors
    s = edge_scaffold()
    seqs = [w["seq"] for w in G["windows"]] + [s[1300:1900], s[2400:3600], s]
    eng.load(seqs)
    X = windowVectors(eng, range(len(seqs)), [0] * len(seqs), [len(q) for q in seqs], 1, 6)
    _labels, old = symmetricCounts([(str(i), q) for i, q in enumerate(seqs)], 1, 6)
    assert X.tolist() == old.tolist()
    with pytest.raises(ValueError, match="30 % unresolved"):
        windowVectors(eng, [len(seqs) - 1], [2540], [2840], 1, 6)
