"""Model-based walk over one context's calls.  A real Engine and an oracle-backed model (tests/residency_model.py) go side by side
through seeded random sequences of loads, stages, commits, profile calls, scans, read-backs and calls the library must refuse; every
observable is compared after every call that produces one:
  - raw profile, symmetric profile and the three metadata values: the model's (oracle/frisk_oracle_np.py), exactly;
  - seq_count / seq_len / seq_name / padded_len: the model's, after every step;
  - packed arrays, the 2-bit form and read-back sequences: those of a second context that only loads the same batch, exactly;
  - scan rows: bit-identical to that second context scanning the same batch with the same finished profile, and the C oracle's
    at the differential fuzz's tolerances (integers, GC and RIP bit-exact, KLD within 1e-11);
  - refused calls: the expected FRISK_E_* code, and the model's state unchanged.
The walk produces the orderings one hand-written test does not: a stage right behind a commit, a loader right behind a streamed
commit (its code pieces possibly still on their way), batches of exactly the previous batch's lengths (no device buffer is
reallocated), a profile added to after its finalisation.  One context per word-size configuration, so that every phase-A form of
profile_add and every scan kernel is walked: (1, 4) and (2, 6) one-half LDS profile and scan_kernel.h; (1, 8) two-half and
one-pass profile, the narrow-counter K = 8 forms; (6, 8) the K = 8 form of scan_kernel.h; (1, 10) global-atomic profile and
scan_big.  A failure names the configuration, the seed, the step and the log of calls so far: the walk replays from them."""
import ctypes as C
import os

import numpy as np
import pytest

from frisk_amd import _ffi
from oracle import frisk_oracle_c as OC

from residency_model import Batch, Model, canonical

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 4), (2, 6), (1, 8), (6, 8), (1, 10)]
SEEDS = range(6)
STEPS = 160
ACGT = np.frombuffer(b"ACGT", np.uint8)
FASTA_ODD = np.frombuffer(b"NnRYKMSWBDHVrykm", np.uint8)
ANY_ODD = np.frombuffer(b"NnRYKMSWBDHVrykmswbdhv-*.x", np.uint8)
IS_ACGT = np.zeros(256, bool)
IS_ACGT[list(b"ACGTacgt")] = True
IS_LOW = np.zeros(256, bool)
IS_LOW[list(b"acgt")] = True
# (weight, name): every operation also occurs at least once in every walk
OPS = [(4, "load"), (4, "synth"), (2, "load_fasta"), (3, "load_shard"),
       (3, "stage"), (2, "stage_packed"), (4, "stage_2bit"), (4, "commit"), (2, "stream_then_load"), (2, "commit_then_stage"),
       (2, "reset"), (6, "add"), (4, "add_range"), (2, "raw"), (1, "set_raw"), (5, "finalize"), (2, "get"), (1, "set_profile"),
       (6, "scan"), (1, "scan_ivom"), (2, "read_seq"), (2, "export_packed"), (2, "export_2bit"),
       (1, "commit_twice"), (1, "scan_unfinalised"), (1, "bad_range"), (1, "bad_runs"), (1, "negative_load")]


class Refused(Exception):
    pass


def expect_error(code, fn, *a, **kw):
    """Run fn; it must raise FriskHipError(code), or succeed when code is None."""
    try:
        out = fn(*a, **kw)
    except _ffi.FriskHipError as err:
        assert code is not None and err.code == code, "raised %r, expected %s" % (err, code)
        raise Refused() from None
    assert code is None, "succeeded, expected error %d" % code
    return out


def random_seq(rng, n, odd=ANY_ODD):
    s = rng.choice(ACGT, n, p=rng.dirichlet([2, 2, 2, 2]))
    for _ in range(int(rng.integers(0, 9)) if n else 0):
        a = int(rng.integers(0, n))
        ln = int(rng.choice([1, 7, 8, 31, 32, 33, 64, 97, 500, 1500]))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            s[a:a + ln] = ord("N")
        elif kind == 1:
            s[a:a + ln] |= 0x20                                             # soft-masked
        elif kind == 2:
            s[a:a + ln] = rng.choice(odd, len(s[a:a + ln]))
        elif kind == 3:
            s[a:a + ln] = s[a]                                              # low complexity
        else:
            s[a:a + ln] = ord("n")
    return s.tobytes()


def random_lens(rng, budget=200_000):
    lens = []
    for _ in range(int(rng.integers(0, 7)) if rng.random() < 0.05 else int(rng.integers(1, 7))):
        lens.append(int(rng.choice([0, 1, 2, 31, 32, 33, 63, 64, 65, 700, int(rng.integers(2_000, 60_000))])))
    while sum(lens) > budget:
        lens[int(np.argmax(lens))] //= 2
    return lens


def awkward_seqs(rng):
    s = bytearray(random_seq(rng, 6_000))
    for a in range(0, 6_000 - 200, 160):                                # runs across word boundaries
        s[max(0, a - 17):a + 19] = b"N" * len(s[max(0, a - 17):a + 19])
        s[a + 40:a + 77] = bytes(c | 0x20 for c in s[a + 40:a + 77])
        s[a + 100] = ord("n")
    # (every byte value but 0: a NUL is the ASCII path's PAD marker, frisk_device.h)
    return [bytes(range(1, 256)) * 2, b"", bytes(s), b"A", b"", b"n" * 33 + b"acgt" * 20 + b"N" * 95, b"ACGTacgtNnRYKMSWBDHV-*"]


def dense_masks(B):
    """The two masks of batch B as dense bitmaps (P / 32 words, real bases only; first position most significant)."""
    inv, low = np.zeros(B.padded, bool), np.zeros(B.padded, bool)
    for s, o in zip(B.seqs, B.off):
        a = np.frombuffer(s, np.uint8)
        inv[o:o + len(s)] = ~IS_ACGT[a]
        low[o:o + len(s)] = IS_LOW[a]
    pack = lambda m: np.packbits(m).view(">u4").astype(np.uint32)         # noqa: E731
    return pack(inv), pack(low)


class Walk:
    def __init__(self, kmin, kmax, seed, tmp):
        from frisk_amd import Engine
        self.kmin, self.kmax, self.seed, self.tmp = kmin, kmax, seed, tmp
        self.rng = np.random.default_rng([seed, kmin, kmax])
        self.e = Engine(kmin, kmax)
        self.ref = Engine(kmin, kmax)            # loads, profiles (profile_set) and scans only
        self.ref_batch = self.ref_final = None
        self.m = Model(kmin, kmax)
        self.log = []
        self.n_files = self.n_pinned = 0
        self.rows_checked = 0

    def close(self):
        self.e.close()
        self.ref.close()

    def note(self, s):
        self.log.append(s)

    # ------------------------------------------------------------------ batches
    def new_batch(self, same_lens=True):
        rng, R = self.rng, self.m.resident
        if same_lens and R is not None and not R.tiled and rng.random() < 0.3:
            lens = list(R.lens)                                             # no device buffer is reallocated
        elif rng.random() < 0.15:
            return Batch(awkward_seqs(rng))
        else:
            lens = random_lens(rng)
        return Batch([random_seq(rng, n) for n in lens])

    def synth_args(self, lens):
        rng = self.rng
        kw = dict(island_frac=float(rng.choice([0.0, 0.02, 0.3])), n_frac=float(rng.choice([0.0, 0.05])),
                  lower_frac=float(rng.choice([0.0, 0.1, 0.4])), repeats_per_kb=float(rng.choice([0.0, 0.5, 2.0])))
        if rng.random() < 0.4:
            kw.update(period_mix=float(rng.choice([0.3, 1.0])), sat_frac=float(rng.choice([0.0, 0.2, 0.6])))
        return int(rng.integers(1, 1 << 40)), kw

    def write_fasta(self, records, names):
        self.n_files += 1
        path = os.path.join(self.tmp, "w%d.fa" % self.n_files)
        with open(path, "wb") as fh:
            for name, s in zip(names, records):
                fh.write(b">" + name.encode() + b" walk record\n")
                for a in range(0, len(s), 60):
                    fh.write(s[a:a + 60] + b"\n")
        return path

    def fasta_batch(self):
        rng = self.rng
        lens = [n for n in random_lens(rng) if n > 0] or [100]
        records = [random_seq(rng, n, FASTA_ODD) for n in lens]
        names = ["rec%d_%d" % (self.n_files, i) for i in range(len(records))]
        return records, names, self.write_fasta(records, names)

    # ------------------------------------------------------------------ checks
    def ref_load(self, B):
        if self.ref_batch is not B:
            if B.tiled:
                sh = B.shard
                self.ref.load_fasta_shard(sh["path"], sh["w"], sh["inc"], sh["rank"], sh["world"], scaffolds_all=sh["scaffolds_all"],
                                          index=sh["index"])
            else:
                self.ref.load(B.seqs)
            self.ref_batch, self.ref_final = B, None
        return self.ref

    def check_meta(self):
        lib, ctx, B = self.e._lib, self.e._ctx, self.m.resident
        assert lib.frisk_seq_count(ctx) == len(B.lens), "seq_count"
        for s in range(len(B.lens)):
            assert lib.frisk_seq_len(ctx, s) == B.lens[s], "seq_len(%d)" % s
            assert lib.frisk_seq_name(ctx, s).decode("latin1") == B.names[s], "seq_name(%d)" % s
        assert lib.frisk_seq_len(ctx, len(B.lens)) == -1, "seq_len past the batch"
        assert self.e.padded_len == B.padded, "padded_len"

    def check_raw(self):
        assert np.array_equal(self.e.profile_raw(), self.m.raw), "raw profile"

    def check_resident(self):
        ref = self.ref_load(self.m.resident)
        for a, b, nm in zip(self.e.export_packed(), ref.export_packed(), ("codes", "inv", "low")):
            assert np.array_equal(a, b), "export_packed: " + nm

    def scan_args(self):
        rng, B = self.rng, self.m.resident
        if B.tiled:
            w, inc, sa = B.shard["w"], B.shard["inc"], B.shard["scaffolds_all"]
        else:
            w = int(rng.choice([400, 1000, 2500]))
            inc, sa = max(1, int(w * rng.choice([0.25, 0.5, 1.0, 1.3]))), bool(rng.integers(0, 2))
        return w, inc, sa

    def ranged(self, n, most):
        rng = self.rng
        c0, c1 = 0, -1
        if rng.random() < 0.5 and n:
            c0 = int(rng.integers(0, n + 1))
            c1 = int(rng.integers(c0, n + 1))
        if most is not None and (c1 if c1 >= 0 else n) - c0 > most:
            c1 = c0 + most
        return c0, c1

    # ------------------------------------------------------------------ operations
    def op_load(self):
        B = self.new_batch()
        self.note("load %s" % B.describe())
        self.e.load(B.seqs)
        self.m.load(B)

    def op_synth(self):
        R = self.m.resident
        lens = list(R.lens) if (R is not None and not R.tiled and self.rng.random() < 0.4) else random_lens(self.rng)
        seed, kw = self.synth_args(lens)
        self.note("synth lens=%s seed=%d %s" % (lens, seed, kw))
        self._synth(lens, seed, kw)

    def _synth(self, lens, seed, kw):
        from frisk_amd import synth
        self.e.synth(lens, seed, **kw)
        self.m.load(Batch([synth.scaffold(n, seed, i, **kw) for i, n in enumerate(lens)]))

    def op_load_fasta(self):
        records, names, path = self.fasta_batch()
        self.note("load_fasta %s lens=%s" % (os.path.basename(path), [len(s) for s in records]))
        from frisk_amd.fasta import readFasta
        got = self.e.load_fasta(path)
        want_names, want_seqs = readFasta(path)
        assert got == want_names == names, "load_fasta names"
        self.m.load(Batch([s.encode() if isinstance(s, str) else s for s in want_seqs], names=want_names))

    def op_load_shard(self):
        from frisk_amd.distributed import plan_tiles
        from frisk_amd.fasta import writeFastaIndex
        rng = self.rng
        records, names, path = self.fasta_batch()
        w = int(rng.choice([400, 1000, 2500]))
        inc, sa = max(1, int(w * rng.choice([0.25, 0.5, 1.0]))), bool(rng.integers(0, 2))
        world = int(rng.integers(2, 5))
        rank = int(rng.integers(0, world))
        index = None
        if rng.random() < 0.5 and writeFastaIndex(path, path + ".fai") is not None:
            index = path + ".fai"
        self.note("load_fasta_shard %s lens=%s w=%d inc=%d all=%s rank=%d world=%d index=%s" % (
            os.path.basename(path), [len(s) for s in records], w, inc, sa, rank, world, index is not None))
        got_names, (c0, c1) = self.e.load_fasta_shard(path, w, inc, rank, world, scaffolds_all=sa, index=index)
        (w0, w1), tiles = plan_tiles([len(s) for s in records], w, inc, sa, self.kmax, rank, world)
        assert got_names == names and (c0, c1) == (w0, w1), "shard names / candidate range"
        shard = dict(path=path, w=w, inc=inc, scaffolds_all=sa, rank=rank, world=world, index=index, c0=c0, c1=c1)
        self.m.load(Batch([records[t["scaf"]][t["base0"]:t["end"]] for t in tiles], names=names, tiles=tiles, shard=shard,
                          records=records))

    def _stage_any(self, B, form=None):
        """Stage batch B in one of the four forms; returns a description."""
        rng, e = self.rng, self.e
        form = form or str(rng.choice(["ascii", "ascii_pinned", "packed", "2bit"]))
        if form == "ascii":
            e.stage(B.seqs)
        elif form == "ascii_pinned":
            self.n_pinned += 1
            buf = e.host_array("walk%d" % self.n_pinned, max(sum(len(s) for s in B.seqs), 1))
            views, o = [], 0
            for s in B.seqs:
                buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
                views.append(buf[o:o + len(s)])
                o += len(s)
            e.stage(views)
        elif form == "packed":
            codes, inv, low = [a.copy() for a in self.ref_load(B).export_packed()]
            e.stage_packed(codes, inv, low, B.lens)
        else:
            pinned = bool(rng.integers(0, 2))
            codes, ri, rl, lens = e.pack_2bit(B.seqs, pinned=pinned)
            assert lens == B.lens
            dense = int(rng.integers(0, 4))
            if dense:
                inv_d, low_d = dense_masks(B)
                ri = inv_d if dense & 1 else ri
                rl = low_d if dense & 2 else rl
            piece = int(rng.choice([0, 32, 64, 4096 + 32, 33, 97, 1001]))
            e.stage_2bit(codes, ri, rl, lens, piece_bases=piece)
            form = "2bit(pinned=%s dense=%d piece_bases=%d)" % (pinned, dense, piece)
        self.m.stage(B)
        return form

    def op_stage(self, form=None):
        B = self.new_batch()
        self.note("stage %s" % B.describe())
        self.log[-1] += " as " + self._stage_any(B, form)

    def op_stage_packed(self):
        self.op_stage("packed")

    def op_stage_2bit(self):
        self.op_stage("2bit")

    def op_commit(self, names=None):
        code = None if self.m.staged is not None else _ffi.E_STATE
        if names is None and self.m.staged is not None and self.rng.random() < 0.3:
            names = ["c%d_%d" % (len(self.log), i) for i in range(len(self.m.staged.lens))]
        self.note("commit%s" % (" names" if names else ""))
        try:
            expect_error(code, self.e.commit, names)
        except Refused:
            assert self.m.commit() == _ffi.E_STATE
            return
        staged = self.m.staged
        self.m.commit()
        if names:
            staged.names = list(names)

    def op_stream_then_load(self):
        """A streamed commit, a loader straight behind it: the loader must not be overwritten by the upload's late pieces."""
        rng = self.rng
        B = self.new_batch(same_lens=False)
        codes, ri, rl, lens = self.e.pack_2bit(B.seqs, pinned=True)
        piece = int(rng.choice([32, 64, 97]))
        self.note("stage_2bit %s piece_bases=%d; commit; then a loader" % (B.describe(), piece))
        self.e.stage_2bit(codes, ri, rl, lens, piece_bases=piece)
        self.m.stage(B)
        self.op_commit()
        if rng.random() < 0.5:
            seed, kw = self.synth_args(lens)
            self.note("synth (same lens) seed=%d %s" % (seed, kw))
            self._synth(list(lens), seed, kw)
        else:
            B2 = Batch([random_seq(rng, n) for n in lens])
            self.note("load (same lens)")
            self.e.load(B2.seqs)
            self.m.load(B2)
        self.check_resident()

    def op_commit_then_stage(self):
        if self.m.staged is None:
            self.op_stage()
        self.op_commit()
        self.op_stage()

    def op_reset(self):
        self.note("profile_reset")
        self.e.profile_reset()
        self.m.reset()

    def op_add(self, one_pass=None):
        rng = self.rng
        mask = bool(rng.integers(0, 2))
        one_pass = bool(rng.integers(0, 2)) if one_pass is None else one_pass
        self.note("profile_add(mask_host=%s, one_pass=%s)" % (mask, one_pass))
        self.e.profile_add(mask_host=mask, one_pass=one_pass)
        assert self.m.add(mask) is None
        if rng.random() < 0.5:
            self.check_raw()

    def op_add_range(self):
        rng, B = self.rng, self.m.resident
        P = B.padded
        kind = int(rng.integers(0, 4))
        if kind == 0:                                                   # word-aligned
            p0 = int(rng.integers(0, P // 32 + 1)) * 32
            p1 = int(rng.integers(p0 // 32, P // 32 + 1)) * 32
        elif kind == 1:                                                 # empty
            p0 = p1 = int(rng.integers(0, P + 1))
        else:                                                           # anywhere: cuts scaffolds, not word-aligned
            p0 = int(rng.integers(0, P + 1))
            p1 = int(rng.integers(p0, P + 1))
        mask, one_pass = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        self.note("profile_add(mask_host=%s, one_pass=%s, %d, %d) of P=%d" % (mask, one_pass, p0, p1, P))
        snap = self.m.snapshot()
        code = self.m.add_error(p0, p1)
        try:
            expect_error(code, self.e.profile_add, mask_host=mask, pos_begin=p0, pos_end=p1, one_pass=one_pass)
        except Refused:
            assert self.m.same_as(snap)
            self.check_raw()
            return
        self.m.add(mask, p0, p1)
        self.check_raw()

    def op_raw(self):
        self.note("profile_raw")
        self.check_raw()

    def op_set_raw(self):
        other = self.new_batch(same_lens=False)
        from oracle import frisk_oracle_np as N
        raw = N.raw_profile(other.enc, self.kmin, self.kmax, bool(self.rng.integers(0, 2)))
        self.note("profile_set_raw (of %s)" % other.describe())
        self.e.profile_set_raw(raw)
        self.m.set_raw(raw)

    def op_finalize(self):
        self.note("profile_finalize")
        self.e.profile_finalize()
        self.m.finalize()
        if self.rng.random() < 0.5:
            self.op_get()

    def op_get(self):
        self.note("profile_get")
        code = self.m.get_error()
        try:
            sym, tl, ex, nn = expect_error(code, self.e.profile_get)
        except Refused:
            return
        assert np.array_equal(sym, self.m.final[0]) and (tl, ex, nn) == self.m.final[1], "profile_get"

    def op_set_profile(self):
        other = self.new_batch(same_lens=False)
        from oracle import frisk_oracle_np as N
        sym, meta = N.genome_profile(other.seqs, self.kmin, self.kmax, bool(self.rng.integers(0, 2)))
        self.note("profile_set (of %s)" % other.describe())
        self.e.profile_set(sym, *meta)
        self.m.set_profile(sym, meta)

    def op_scan(self):
        rng, B = self.rng, self.m.resident
        if self.m.final is None and rng.random() < 0.75:
            self.op_finalize()
        w, inc, sa = self.scan_args()
        rip = self.kmin <= 2 <= self.kmax and bool(rng.integers(0, 2))
        chunks = bool(rng.integers(0, 2))
        bits4 = side4 = False
        if self.kmax == 8:
            form = int(rng.integers(0, 3))
            bits4, side4 = form == 1, form == 2
        code = self.m.scan_error(w, inc, sa)
        n = 0 if code is not None else self.ref_load(B).scan_plan(w, inc, sa)
        c0, c1 = self.ranged(n, 48 if self.kmax > 8 else None)
        kw = dict(rip=rip, scaffolds_all=sa, c0=c0, c1=c1, chunks=chunks, bits4=bits4, side4=side4)
        self.note("scan(%d, %d, %s)" % (w, inc, kw))
        snap = self.m.snapshot()
        try:
            got = expect_error(code, self.e.scan, w, inc, **kw)
        except Refused:
            assert self.m.same_as(snap)
            return
        ref = self.ref_load(B)
        if self.ref_final is not self.m.final:
            sym, meta = self.m.final
            ref.profile_set(sym, *meta)
            self.ref_final = self.m.final
        want = ref.scan(w, inc, **kw)
        assert got.n_candidates == want.n_candidates == n, "candidates"
        for f in ("seq_index", "start", "stop", "status", "kld", "gc") + (("pi", "si", "cri") if rip else ()):
            assert np.array_equal(getattr(got, f), getattr(want, f), equal_nan=True), "rows differ from a context that only loaded: " + f
        # ... and the C oracle's rows (the differential fuzz's tolerances)
        sym, meta = self.m.final
        ig = OC.genome_ivom(sym, meta, self.kmin, self.kmax)
        if B.tiled:
            seqs, off = B.records, B.shard["c0"]
        else:
            seqs, off = B.seqs, 0
        cend = off + (c1 if c1 >= 0 else n)
        exp = OC.scan(seqs, ig, self.kmin, self.kmax, w, inc, scaffolds_all=sa, rip=rip, cand=(off + c0, cend))
        k = np.nonzero(got.kept)[0]
        assert len(k) == len(exp["kld"]), "kept rows vs the C oracle"
        if not len(k):
            return
        assert np.array_equal(got.seq_index[k], exp["seq"]), "seq_index vs the C oracle"
        assert np.array_equal(got.start[k], exp["start"]) and np.array_equal(got.stop[k], exp["stop"]), "start/stop vs the C oracle"
        assert np.array_equal(got.gc[k], exp["gc"], equal_nan=True), "GC vs the C oracle"
        zero = (exp["status"] & OC.ROW_ZERO_DIV) != 0
        assert np.array_equal((got.status[k] & _ffi.ROW_ZERO_WEIGHT) != 0, zero), "zero-weight rows vs the C oracle"
        assert np.array_equal((got.status[k] & _ffi.ROW_NO_MAXMER) != 0, (exp["status"] & OC.ROW_NO_MAXMER) != 0), "no-max-mer rows"
        if rip:
            for col in ("pi", "si", "cri"):
                assert np.array_equal(getattr(got, col)[k], exp[col], equal_nan=True), col + " vs the C oracle"
        ok = ~zero
        if ok.any():
            assert np.max(np.abs(got.kld[k][ok] - exp["kld"][ok])) <= 1e-11, "KLD vs the C oracle"
        self.rows_checked += len(k)

    def op_scan_ivom(self):
        if self.kmax > 6:
            return self.op_scan()
        B = self.m.resident
        if self.m.final is None and self.rng.random() < 0.75:
            self.op_finalize()
        w, inc, sa = self.scan_args()
        code = self.m.scan_error(w, inc, sa)
        n = 0 if code is not None else self.ref_load(B).scan_plan(w, inc, sa)
        c0, c1 = self.ranged(n, 64)
        self.note("scan_ivom(%d, %d, all=%s, %d, %d)" % (w, inc, sa, c0, c1))
        try:
            wi, gi = expect_error(code, self.e.scan_ivom, w, inc, scaffolds_all=sa, c0=c0, c1=c1)
        except Refused:
            return
        ref = self.ref_load(B)
        if self.ref_final is not self.m.final:
            ref.profile_set(self.m.final[0], *self.m.final[1])
            self.ref_final = self.m.final
        rw, rg = ref.scan_ivom(w, inc, scaffolds_all=sa, c0=c0, c1=c1)
        assert np.array_equal(wi, rw, equal_nan=True) and np.array_equal(gi, rg, equal_nan=True), "scan_ivom differs from a context that only loaded"

    def op_read_seq(self):
        rng, B = self.rng, self.m.resident
        if B.tiled:
            self.note("read_seq(0) of a tiled batch")
            try:
                expect_error(_ffi.E_STATE, self.e.read_seq, 0, 0, 0)
            except Refused:
                return
        if not B.seqs:
            return
        s = int(rng.integers(0, len(B.seqs)))
        n = len(B.seqs[s])
        a = int(rng.integers(0, n + 1))
        b = int(rng.integers(a, n + 1)) if rng.random() < 0.5 else n
        self.note("read_seq(%d, %d, %d)" % (s, a, b - a))
        assert self.e.read_seq(s, a, b - a) == canonical(B.seqs[s][a:b]), "read_seq"

    def op_export_packed(self):
        self.note("export_packed")
        self.check_resident()

    def op_export_2bit(self):
        pinned = bool(self.rng.integers(0, 2))
        self.note("export_2bit(pinned=%s)" % pinned)
        got = self.e.export_2bit(pinned=pinned)
        want = self.ref_load(self.m.resident).export_2bit()
        for a, b, nm in zip(got, want, ("codes", "inv_runs", "low_runs")):
            assert np.array_equal(a, b), "export_2bit: " + nm

    def op_commit_twice(self):
        self.op_stage()
        self.op_commit()
        self.op_commit()                         # nothing staged: FRISK_E_STATE, the batch just committed stays resident
        self.check_resident()

    def op_scan_unfinalised(self):
        """A profile added to after its finalisation is not finished: a scan must be refused until the next finalisation."""
        self.op_finalize()
        self.op_add()
        self.op_scan()

    def op_bad_range(self):
        B = self.m.resident
        p0, p1 = [(0, B.padded + 32), (-1, 5), (10, 5), (5, -1), (B.padded + 1, B.padded + 1)][int(self.rng.integers(0, 5))]
        self.note("profile_add(%d, %d): refused" % (p0, p1))
        snap = self.m.snapshot()
        try:
            expect_error(_ffi.E_ARG, self.e.profile_add, pos_begin=p0, pos_end=p1)
        except Refused:
            pass
        assert self.m.same_as(snap)
        self.check_raw()

    def op_bad_runs(self):
        B = self.new_batch(same_lens=False)
        codes, ri, rl, lens = self.e.pack_2bit(B.seqs, pinned=False)
        bad = [np.array([[5, 3]]), np.array([[0, B.padded + 1]]), np.array([[-4, 2]])][int(self.rng.integers(0, 3))]
        self.note("stage_2bit with the run list %s: refused" % bad.tolist())
        try:
            expect_error(_ffi.E_ARG, self.e.stage_2bit, codes, bad, rl, lens)
        except Refused:
            pass
        self.m.stage_refused()
        self.check_resident()

    def op_negative_load(self):
        """frisk_seq_load / frisk_seq_synth2 with a negative length: FRISK_E_ARG, and nothing of the resident batch changes."""
        rng = self.rng
        n = int(rng.integers(1, 9))
        lens = [int(rng.integers(0, 300)) for _ in range(n)]
        lens[int(rng.integers(0, n))] = -1
        bufs = [b"ACGT" * 100 for _ in range(n)]
        arr, clens = (C.c_char_p * n)(*bufs), (C.c_int64 * n)(*lens)
        lib, ctx = self.e._lib, self.e._ctx
        synth = bool(rng.integers(0, 2))
        self.note("%s lens=%s: refused" % ("frisk_seq_synth2" if synth else "frisk_seq_load", lens))
        snap = self.m.snapshot()
        if synth:
            rc = lib.frisk_seq_synth2(ctx, clens, n, C.c_uint64(7), 0.02, 0.0, 0.0, 0.0, 0.0, 0.0)
        else:
            rc = lib.frisk_seq_load(ctx, arr, clens, n)
        assert rc == _ffi.E_ARG, rc
        assert self.m.same_as(snap)
        self.check_meta()
        self.check_resident()

    # ------------------------------------------------------------------ the walk
    def schedule(self, steps):
        names = [nm for _, nm in OPS]
        p = np.array([wt for wt, _ in OPS], float)
        extra = list(self.rng.choice(names, max(0, steps - len(names)), p=p / p.sum()))
        order = names + extra
        self.rng.shuffle(order)
        return ["load"] + [str(x) for x in order]

    def run(self, steps):
        for step, name in enumerate(self.schedule(steps)):
            start = len(self.log)
            try:
                getattr(self, "op_" + name)()
                self.check_meta()
            except Exception as err:                                   # noqa: BLE001 - re-raised with the replay information
                raise AssertionError("config (%d, %d) seed %d: step %d (%s) failed: %r\nlog of calls (step %d starts at line %d):\n%s" % (
                    self.kmin, self.kmax, self.seed, step, name, err, step, start,
                    "\n".join("%4d  %s" % (i, s) for i, s in enumerate(self.log)))) from err


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kmin,kmax", CONFIGS)
def test_residency_walk(tmp_path, kmin, kmax, seed):
    w = Walk(kmin, kmax, seed, str(tmp_path))
    try:
        w.run(STEPS)
    finally:
        w.close()
    assert w.rows_checked > 0
