"""One deterministic test per residency defect the model-based walk (tests/test_gpu_residency_walk.py) was written to find:
  1. a loader straight behind a streamed commit refills the resident slot while the upload's code pieces may still be in flight;
  2. FRISK_PROFILE_ONE_PASS must never act as --maskHost, on any path (kmax > 8, piece by piece, ranges);
  3. a refused load (a negative length) must leave the resident batch, its lengths and its names alone;
  4. page-locked arrays Engine hands out (pack_2bit / export_2bit / export_packed) belong to the caller: no later call rewrites them."""
import ctypes as C
import gc

import numpy as np
import pytest

from frisk_amd import _ffi
from oracle import frisk_oracle_np as N

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


def soft_masked(rng, n):
    s = rng.choice(ACGT, n)
    for a in range(0, n - 400, 700):                 # soft-masked runs of every length up to 300, across word boundaries
        s[a + 13:a + 13 + (a // 7) % 300 + 1] |= 0x20
    s[n // 3:n // 3 + 50] = ord("N")
    odd = np.frombuffer(b"acgtnRYac", np.uint8)
    s[n // 2:n // 2 + 9] = odd[:len(s[n // 2:n // 2 + 9])]
    return s.tobytes()


def write_fasta(path, names, seqs, width=60):
    with open(path, "wb") as fh:
        for name, s in zip(names, seqs):
            fh.write(b">" + name.encode() + b"\n")
            for a in range(0, len(s), width):
                fh.write(s[a:a + width] + b"\n")


def profile_raw(e, **kw):
    e.profile_reset()
    e.profile_add(**kw)
    return e.profile_raw()


# ---------------------------------------------------------------------------------------------------------------- defect 1
@pytest.mark.parametrize("loader", ["synth", "load", "shard", "shard_indexed"])
def test_loader_behind_streamed_commit_is_not_overwritten(tmp_path, loader):
    """A 64 Mb batch staged in the 0.25 B/base form from page-locked codes in small pieces (4 096 copies), committed, and at once
    replaced by a loader writing a DIFFERENT batch of the SAME lengths into the same slot (no reallocation): the resident words and
    the profile must be the new batch's - the loader waits, on the device, for the upload's last piece.  synth has no host upload
    in front of its pack kernel: the widest window."""
    from frisk_amd import Engine
    from frisk_amd.fasta import writeFastaIndex
    lens = [40_000_000, 24_000_017]
    kw = dict(island_frac=0.1, n_frac=0.02, lower_frac=0.2, repeats_per_kb=0.5)
    with Engine(1, 8) as e, Engine(1, 8) as ref:
        # the batch the loader writes, and what a context that only loads it holds
        ref.synth(lens, 202, **kw)
        if loader == "synth":
            want = [a.copy() for a in ref.export_packed()]
        else:
            seqs_c = [ref.read_seq(i) for i in range(len(lens))]
            if loader == "load":
                ref.load(seqs_c)
            else:
                fa = str(tmp_path / "c.fa")
                write_fasta(fa, ["c0", "c1"], seqs_c)
                index = str(tmp_path / "c.fa.fai") if loader == "shard_indexed" else None
                if index is not None:
                    assert writeFastaIndex(fa, index) == 2
                ref.load_fasta_shard(fa, 5000, 1000, 0, 1, index=index)
                assert ref.seq_lens == lens
            want = [a.copy() for a in ref.export_packed()]
        want_raw = profile_raw(ref)
        # batch A, streamed in
        e.synth(lens, 101, **kw)
        codes, ri, rl = e.export_2bit(pinned=True)
        e.synth(lens, 303, **kw)                    # (another batch in the first slot)
        e.stage_2bit(codes, ri, rl, lens, piece_bases=1 << 14)
        e.commit()
        if loader == "synth":
            e.synth(lens, 202, **kw)
        elif loader == "load":
            e.load(seqs_c)
        else:
            e.load_fasta_shard(fa, 5000, 1000, 0, 1, index=index)
            assert e.shard_index == index
        assert e.padded_len == ref.padded_len              # (one rank's tiles are the whole scaffolds: the same layout as A)
        got = e.export_packed()
        for a, b, nm in zip(got, want, ("codes", "inv", "low")):
            assert np.array_equal(a, b), "%s: the resident %s words are not the loaded batch's" % (loader, nm)
        assert np.array_equal(profile_raw(e), want_raw), loader


# ---------------------------------------------------------------------------------------------------------------- defect 2
@pytest.mark.parametrize("kmin,kmax", [(1, 9), (2, 10), (1, 12)])
def test_one_pass_never_masks(kmin, kmax):
    """FRISK_PROFILE_ONE_PASS (a test hook of the K = 8 form) with and without --maskHost at kmax > 8, on soft-masked sequence:
    whole, over position ranges and over a streamed commit (piece by piece), the counts are raw_profile's with the mask asked
    for - never the masked ones without it."""
    from frisk_amd import Engine
    rng = np.random.default_rng(kmax)
    seqs = [soft_masked(rng, 21_000), soft_masked(rng, 6_003), b"acgtACGT" * 40]
    want = {m: N.raw_profile(seqs, kmin, kmax, m) for m in (False, True)}
    assert not np.array_equal(want[False], want[True])
    with Engine(kmin, kmax) as e:
        e.load(seqs)
        for mask in (False, True):
            for one_pass in (True, False):
                assert np.array_equal(profile_raw(e, mask_host=mask, one_pass=one_pass), want[mask]), ("whole", mask, one_pass)
        P = e.padded_len
        offs = np.cumsum([0] + [len(s) + 1 for s in seqs])[:-1]
        cuts = [(0, 1000), (1000, 12_345), (21_003, 21_040), (12_345, P)]   # (the third is short and cuts scaffold 1's start)
        for mask in (False, True):
            e.profile_reset()
            for a, b in cuts:
                e.profile_add(mask_host=mask, pos_begin=a, pos_end=b, one_pass=True)
            want_r = sum(N.raw_profile(seqs, kmin, kmax, mask, [(a - o, b - o) for o in offs]) for a, b in cuts)
            assert np.array_equal(e.profile_raw(), want_r), ("ranges", mask)
        codes, ri, rl, lens = e.pack_2bit(seqs)
        for mask in (False, True):
            e.stage_2bit(codes, ri, rl, lens, piece_bases=4096)
            e.commit()
            assert np.array_equal(profile_raw(e, mask_host=mask, one_pass=True), want[mask]), ("streamed", mask)


# ---------------------------------------------------------------------------------------------------------------- defect 3
def test_refused_load_leaves_the_resident_batch(tmp_path):
    """frisk_seq_load and frisk_seq_synth2 with a negative length and fewer scaffolds than are resident: FRISK_E_ARG, and every
    observable of the resident batch - count, lengths, names, sequence, profile, rows - is what it was."""
    from frisk_amd import Engine
    rng = np.random.default_rng(3)
    seqs = [soft_masked(rng, n) for n in (12_000, 7_001, 900, 30_000, 5)]
    names = ["scaf%d" % i for i in range(len(seqs))]
    fa = str(tmp_path / "r.fa")
    write_fasta(fa, names, seqs)
    with Engine(1, 8) as e:
        assert e.load_fasta(fa) == names
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        raw0, prof0, rows0, padded0 = e.profile_raw(), e.profile_get(), e.scan(1000, 250, rip=True), e.padded_len
        lib, ctx = e._lib, e._ctx
        for call in ("load", "synth2"):
            lens = (C.c_int64 * 2)(4_000, -1)
            if call == "load":
                rc = lib.frisk_seq_load(ctx, (C.c_char_p * 2)(b"A" * 4_000, b""), lens, 2)
            else:
                rc = lib.frisk_seq_synth2(ctx, lens, 2, C.c_uint64(9), 0.02, 0.0, 0.0, 0.0, 0.0, 0.0)
            assert rc == _ffi.E_ARG, (call, rc)
            assert lib.frisk_seq_count(ctx) == len(seqs), call
            for i, s in enumerate(seqs):                # (in ascending order: index 0 is the first a refused layout rewrote)
                assert lib.frisk_seq_len(ctx, i) == len(s), (call, i)
                assert lib.frisk_seq_name(ctx, i).decode() == names[i], (call, i)
            assert e.padded_len == padded0, call
            for i, s in enumerate(seqs):
                assert e.read_seq(i, 0, len(s)) == bytes(c if c in b"ACGTacgt" else ord("N") for c in s), (call, i)
            assert np.array_equal(e.profile_raw(), raw0), call
            rows = e.scan(1000, 250, rip=True)
            for f in ("seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri"):
                assert np.array_equal(getattr(rows, f), getattr(rows0, f), equal_nan=True), (call, f)
            e.profile_reset(); e.profile_add(); e.profile_finalize()
            assert np.array_equal(e.profile_raw(), raw0), call
            sym, tl, ex, nn = e.profile_get()
            assert np.array_equal(sym, prof0[0]) and (tl, ex, nn) == prof0[1:], call


# ---------------------------------------------------------------------------------------------------------------- defect 4
def test_pinned_results_belong_to_the_caller():
    """a = pack_2bit(A, pinned=True) stays A's through a second pack_2bit, export_2bit and export_packed (page-locked each), and
    a batch staged from `a` is still A after B is packed before any synchronising call."""
    from frisk_amd import Engine
    from frisk_amd.engine import pack_2bit_host
    rng = np.random.default_rng(4)
    A = [soft_masked(rng, 50_000), soft_masked(rng, 3_000)]
    B = [rng.choice(ACGT, 30_000).tobytes()]           # smaller, fewer runs: a shared buffer would be reused, not reallocated
    B[0] = B[0][:100] + b"acgtN" + B[0][105:]
    want_a, want_b = pack_2bit_host(A), pack_2bit_host(B)
    with Engine(1, 8) as e, Engine(1, 8) as ref:
        ref.load(A)
        want_resident = [x.copy() for x in ref.export_packed()]
        n_owned = len(getattr(e, "_owned", ()))             # page-locked buffers the engine has handed out so far
        a = e.pack_2bit(A, pinned=True)
        b = e.pack_2bit(B, pinned=True)
        e.load(B)
        x = e.export_2bit(pinned=True)
        p = e.export_packed(pinned=True)
        p_copy = [y.copy() for y in p]
        for got, want, nm in zip(a[:3], want_a[:3], ("codes", "inv_runs", "low_runs")):
            assert np.array_equal(got, want), "a." + nm + " was rewritten"
        for got, want in zip(b[:3], want_b[:3]):
            assert np.array_equal(got, want)
        for got, want in zip(x, want_b[:3]):
            assert np.array_equal(got, want)
        e.stage_2bit(*a, piece_bases=64)
        e.commit()
        e.pack_2bit(B, pinned=True)
        e.pack_2bit(A[:1], pinned=True)
        for got, want, nm in zip(e.export_packed(), want_resident, ("codes", "inv", "low")):
            assert np.array_equal(got, want), "resident " + nm
        for got, want in zip(p, p_copy):
            assert np.array_equal(got, want), "an export_packed(pinned=True) result was rewritten"
        del a, b, x, p, got, want
        gc.collect()
        assert len(e._owned) <= n_owned + 3                 # (the batch staged last keeps its arrays)
