"""Oracle-backed model of one context's state (include/frisk_hip.h): the resident batch, the staged batch, the raw profile and the
finalised profile, and the error each call must raise.  tests/test_gpu_residency_walk.py drives a real Engine and this model side
by side.  Test infrastructure only: every count comes from oracle/frisk_oracle_np.py, every tile from
frisk_amd.distributed.plan_tiles (the specification of frisk_fasta_load_shard)."""
import numpy as np

from frisk_amd import _ffi
from oracle import frisk_oracle_np as N


def canonical(seq):
    """What frisk_seq_read returns for a scaffold: A/T/G/C, a/t/g/c, N for everything else."""
    return bytes(c if c in b"ACGTacgt" else ord("N") for c in seq)


class Batch:
    """A batch as the library holds it: `seqs` are the resident sequences (tiles for a sharded load); `names` / `lens` are what
    frisk_seq_name / frisk_seq_len report (every record of the FASTA for a sharded load)."""
    _next = 0

    def __init__(self, seqs, names=None, tiles=None, shard=None, records=None):
        Batch._next += 1
        self.key = Batch._next
        self.seqs = [bytes(s) for s in seqs]
        self.enc = [N.Encoded(s) for s in self.seqs]
        self.off, pos = [], 0
        for s in self.seqs:
            self.off.append(pos)
            pos += len(s) + 1
        self.padded = max(32, (pos + 31) // 32 * 32)
        self.tiles = tiles                  # plan_tiles' dicts, or None
        self.shard = shard                  # dict(path, w, inc, scaffolds_all, rank, world, index, c0, c1)
        self.records = records              # all records of the FASTA (a sharded load)
        if tiles is not None:
            self.names, self.lens = list(names), [len(r) for r in records]
        else:
            self.names = list(names) if names is not None else [""] * len(self.seqs)
            self.lens = [len(s) for s in self.seqs]

    @property
    def tiled(self):
        return self.tiles is not None

    def describe(self):
        if self.tiled:
            return "shard(rank %d/%d w=%d inc=%d all=%s index=%s tiles=%s)" % (
                self.shard["rank"], self.shard["world"], self.shard["w"], self.shard["inc"], self.shard["scaffolds_all"],
                self.shard["index"] is not None, [len(s) for s in self.seqs])
        return "lens=%s" % [len(s) for s in self.seqs]


class Model:
    def __init__(self, kmin, kmax):
        self.kmin, self.kmax = kmin, kmax
        self.nprof = N.profile_len(kmin, kmax)
        self.resident = None
        self.staged = None
        self.raw = np.zeros(self.nprof + 4, np.int64)
        self.final = None                   # (sym, (totalLen, exMax, nnTotal)) or None: not finalised
        self._raw_cache = {}

    def snapshot(self):
        return (self.resident, self.staged, self.raw.copy(), self.final)

    def same_as(self, snap):
        r, s, raw, fin = snap
        return (self.resident is r and self.staged is s and np.array_equal(self.raw, raw) and
                (self.final is fin or (fin is not None and self.final is not None and np.array_equal(self.final[0], fin[0])
                                       and self.final[1] == fin[1])))

    # ------------------------------------------------------------------ sequences
    def load(self, batch):
        self.resident = batch

    def stage(self, batch):
        self.staged = batch

    def stage_refused(self):
        self.staged = None                  # a refused stage leaves nothing to commit

    def commit(self):
        """The error the commit must raise (None: it succeeds)."""
        if self.staged is None:
            return _ffi.E_STATE
        self.resident, self.staged = self.staged, None
        return None

    # ------------------------------------------------------------------ phase A
    def reset(self):
        self.raw = np.zeros(self.nprof + 4, np.int64)
        self.final = None

    def add_error(self, p0, p1):
        B = self.resident
        if B is None:
            return _ffi.E_STATE
        if p0 < 0 and p1 < 0:
            return None
        if B.tiled:
            return _ffi.E_ARG                # a tiled batch is profiled as a whole
        if p0 < 0 or p1 > B.padded or p0 > p1:
            return _ffi.E_ARG
        return None

    def counts(self, mask_host, p0=-1, p1=-1):
        """raw_profile of the resident batch over padded positions [p0, p1) (-1, -1: the whole batch, the owned positions of a
        tiled one).  The one-pass hook never enters: it is not a mask."""
        B = self.resident
        key = (B.key, bool(mask_host), p0, p1)
        if key not in self._raw_cache:
            if B.tiled:
                ranges = [(t["own0"] - t["base0"], t["own1"] - t["base0"]) for t in B.tiles]
            elif p0 < 0 and p1 < 0:
                ranges = None
            else:
                ranges = [(p0 - o, p1 - o) for o in B.off]
            self._raw_cache[key] = N.raw_profile(B.enc, self.kmin, self.kmax, bool(mask_host), ranges)
        return self._raw_cache[key]

    def add(self, mask_host, p0=-1, p1=-1):
        err = self.add_error(p0, p1)
        if err is None:
            self.raw = self.raw + self.counts(mask_host, p0, p1)
            self.final = None
        return err

    def set_raw(self, raw):
        self.raw = np.asarray(raw, np.int64).copy()
        self.final = None

    def finalize(self):
        sym, meta = N.finalize_raw(self.raw, self.kmin, self.kmax)
        self.final = (sym, tuple(int(v) for v in meta))

    def set_profile(self, sym, meta):
        self.final = (np.asarray(sym, np.int64).copy(), tuple(int(v) for v in meta))

    def get_error(self):
        return _ffi.E_STATE if self.final is None else None

    def scan_error(self, w, inc, scaffolds_all):
        if self.final is None:
            return _ffi.E_STATE
        B = self.resident
        if B.tiled and (w, inc, bool(scaffolds_all)) != (B.shard["w"], B.shard["inc"], B.shard["scaffolds_all"]):
            return _ffi.E_ARG                # the tiles of another window geometry
        return None
