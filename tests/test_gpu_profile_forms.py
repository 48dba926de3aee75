"""Phase A (frisk_profile_add) at its own edges, on every form of profile_kernels.h: the LDS table in one piece (kmax < 8) and in two
halves (kmax = 8), the one-pass 16-bit form (kmax = 8, forced), the global-table form (kmax > 8), and the piecewise launches behind a
streamed upload (profile_plan.h).  Everything phase A writes is an integer sum over positions, so the criterion is exact: the whole raw
array - tables and tail - equals oracle.frisk_oracle_np.raw_profile to the last count.  One batch of about 260 kb, several
65 536-position chunks in one launch: synthetic scaffolds with N runs and soft-masked runs, an empty one, two shorter than a bitmap
word, and one made by hand for the order under test (hand_made)."""
import functools

import numpy as np
import pytest

from oracle import frisk_oracle_np as N

pytestmark = pytest.mark.gpu

LENS = [150_001, 70_000, 40_000, 33, 7, 0]
ORDERS = [(1, 1), (1, 2), (3, 3), (2, 5), (1, 7), (1, 8), (4, 8), (8, 8), (1, 9), (7, 10)]


def hand_made(off, kmax):
    """A scaffold whose first base lies at padded position `off`.  At six word boundaries B (padded multiples of 32, 64 apart) of
    uppercase sequence: an invalid base at a position = 31, at one = 0 and at one = 1 (mod 32); valid runs of kmax - 1, kmax and
    kmax + 1 bases across a boundary, an N on either side; a soft-masked base at a position = 0 (mod 32) (it stops a run under
    --maskHost alone).  The scaffold ends in a run of kmax - 1 bases behind an N."""
    rng = np.random.default_rng(100 + kmax)
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), 32 * 16)
    B = [(off // 32 + 2) * 32 + 64 * k - off for k in range(7)]         # scaffold coordinates of the boundaries
    s[B[0] - 1] = ord("N")
    s[B[1]] = ord("N")
    s[B[2] + 1] = ord("N")
    for b, run in zip(B[3:6], (kmax - 1, kmax, kmax + 1)):
        a = b - max(1, run // 2)                                        # the run is [a, a + run): a < b, and past b where run >= 2
        s[a - 1] = ord("N")
        s[a + run] = ord("N")
    s[B[6]] |= 0x20
    assert B[6] + 1 < len(s) and all((off + b) % 32 == 0 for b in B)
    return s.tobytes() + b"N" + rng.choice(np.frombuffer(b"ACGT", np.uint8), kmax - 1).tobytes()


@functools.lru_cache(maxsize=None)
def batch(kmax, n_synth=len(LENS)):
    """(sequences, the same encoded for the oracle); the synthetic scaffolds are the same for every order"""
    from frisk_amd import synth
    seqs = [synth.scaffold(n, 71, i, island_frac=0.1, n_frac=0.08, lower_frac=0.15) for i, n in enumerate(LENS[:n_synth])]
    if n_synth == len(LENS):
        seqs.append(hand_made(sum(len(s) + 1 for s in seqs), kmax))
    return seqs, [N.Encoded(s) for s in seqs]


@functools.lru_cache(maxsize=None)
def want_raw(kmin, kmax, mask_host, n_synth=len(LENS)):
    raw = N.raw_profile(batch(kmax, n_synth)[1], kmin, kmax, mask_host)
    raw.setflags(write=False)
    return raw


def check_forms(e, kmin, kmax, n_synth=len(LENS)):
    e.load(batch(kmax, n_synth)[0])
    P = e.padded_len
    cuts = [0, 1, 31, 32, 33, 4097, P // 3, P // 2 + 5, P - 1, P]
    assert cuts == sorted(cuts) and P > 3 * 65536            # (a chunk takes at least 65 536 positions: three of them)
    for one_pass in ((False, True) if kmax == 8 else (False,)):
        for mask in (False, True):
            want = want_raw(kmin, kmax, mask, n_synth)
            assert want[-4] == sum(LENS[:n_synth]) + (len(batch(kmax)[0][-1]) if n_synth == len(LENS) else 0)
            e.profile_reset()
            e.profile_add(mask_host=mask, one_pass=one_pass)
            assert np.array_equal(e.profile_raw(), want), ("whole", mask, one_pass)
            for a in (0, 4097, P):                              # an empty range leaves the raw profile as it is
                e.profile_add(mask_host=mask, pos_begin=a, pos_end=a, one_pass=one_pass)
            assert np.array_equal(e.profile_raw(), want), ("empty ranges", mask, one_pass)
            e.profile_reset()                                   # every position in exactly one range: the sum is the whole batch's
            for a, b in zip(cuts[:-1], cuts[1:]):
                e.profile_add(mask_host=mask, pos_begin=a, pos_end=b, one_pass=one_pass)
            assert np.array_equal(e.profile_raw(), want), ("cuts", mask, one_pass)
    assert not np.array_equal(want_raw(kmin, kmax, False, n_synth), want_raw(kmin, kmax, True, n_synth))


@pytest.mark.parametrize("kmin,kmax", ORDERS)
def test_every_form_whole_in_cuts_and_empty(kmin, kmax):
    from frisk_amd import Engine
    with Engine(kmin, kmax) as e:
        check_forms(e, kmin, kmax)


def test_orders_9_to_12_on_two_scaffolds():
    """The widest tables (4^12 bins): the first two scaffolds only."""
    from frisk_amd import Engine
    with Engine(9, 12) as e:
        check_forms(e, 9, 12, n_synth=2)


@pytest.mark.parametrize("piece_bases", [2048, 4096])
@pytest.mark.parametrize("kmin,kmax", [(1, 8), (2, 5)])
def test_streamed_batch_counted_behind_its_pieces(kmin, kmax, piece_bases):
    """stage_2bit / commit and profile_add() straight behind: one launch per upload piece, each a word short of its piece's end."""
    from frisk_amd import Engine
    seqs = batch(kmax)[0]
    with Engine(kmin, kmax) as e:
        codes, ri, rl, lens = e.pack_2bit(seqs)
        for mask in (False, True):
            e.stage_2bit(codes, ri, rl, lens, piece_bases=piece_bases)
            e.commit()
            e.profile_reset()
            e.profile_add(mask_host=mask)
            assert np.array_equal(e.profile_raw(), want_raw(kmin, kmax, mask)), mask
