"""A slid window's geometry by increments (frisk_amd/csrc/win_step.h in scan8_kernel.h): inside a chunk the kernel advances start,
resident position and the ring's row and column from the predecessor's (win_next) instead of computing them from the candidate index
(win_fresh), and stage 1 addresses the sequence by a uniform 64-bit word plus 32-bit lane offsets.  Which of the two a window took
must not show in its row: every column of the chunked scan (Engine.scan(chunks=True): small inputs slide) has the bits of the scan
that counts every window afresh - each window its own launch item, win_fresh only - and the rows agree with the C oracle to 1e-11
(test_gpu_slide.py's bound).  The window-by-window scan runs the new win_fresh and lane arithmetic too (never win_next): what makes
the reference independent of this code is the C oracle - its rows, and the exact start / stop / GC it reports.

The shapes, smallest that still take every path:
  * w = 5000, inc = 1000, one scaffold of 40 inc + w bases: the ring base crosses ITS x COLS = 5120 several times, rb_r = 0 throughout;
  * inc = 1007 and 1010: the general copies, rb_r carries into the column;
  * w = 2048, inc = 100 and w = 600, inc = 8 (100 inc + w bases: the shortest scaffolds are not scanned): the instantiation with 8
    positions per lane;
  * three scaffolds of 9 inc + w + 17 bases: chunks span scaffold ends and jump-back tails;
  * an N run of w / 3 bases and a poly-A run of 40 bases in mid-scaffold: the predecessor of a slid window is dropped / handed on;
  * candidate ranges that start in mid-chunk;
  * the same repeat-rich case through the 8-bit form and the 4-bit form with the side table;
  * K = 6 and K = 7 once each."""
import numpy as np
import pytest

from frisk_amd import _ffi
from frisk_amd.engine import Engine
from oracle import frisk_oracle_c as OC

pytestmark = pytest.mark.gpu

COLS = ("seq_index", "start", "stop", "status", "kld", "gc")
CHUNK = 8                                   # windows per chunk of a scan with chunks=True (scan_schedule.h)
ACGT = np.frombuffer(b"ATGC", dtype=np.uint8)


def _draw(rng, n):
    return rng.choice(ACGT, size=n, p=[0.3, 0.3, 0.2, 0.2])


def _one(w, inc, nwin=40):
    return lambda rng: [_draw(rng, nwin * inc + w)]


def _three(w, inc):
    return lambda rng: [_draw(rng, 9 * inc + w + 17) for _ in range(3)]


def _runs(w, inc):
    def make(rng):
        s = _draw(rng, 40 * inc + w)
        a = 11 * inc + 123
        s[a:a + w // 3] = ord("N")          # 30 % of a window and more: the windows that hold all of it are dropped
        b = 27 * inc + 77
        s[b:b + 40] = ord("A")              # 33 occurrences of one max-mer: wraps a 4-bit counter, the window is handed on
        return [s]
    return make


# name: (kmin, kmax, w, inc, sequences, scans to compare with the fresh one)
CASES = {
    "bench":    (1, 8, 5000, 1000, _one(5000, 1000), [dict(bits4=True)]),
    "inc1007":  (1, 8, 5000, 1007, _one(5000, 1007), [dict(bits4=True)]),
    "inc1010":  (1, 8, 5000, 1010, _one(5000, 1010), [dict(bits4=True)]),
    "w2048":    (1, 8, 2048, 100, _one(2048, 100), [dict(bits4=True)]),
    "w600":     (1, 8, 600, 8, _one(600, 8, 100), [dict(bits4=True)]),      # (a scaffold of up to 1.75 w - inc bases is not scanned)
    "three":    (1, 8, 5000, 1000, _three(5000, 1000), [dict(bits4=True)]),
    "runs":     (1, 8, 5000, 1000, _runs(5000, 1000), [dict(bits4=True), dict(), dict(side4=True)]),
    "k6":       (1, 6, 5000, 1000, _three(5000, 1000), [dict()]),
    "k7":       (2, 7, 2048, 100, _one(2048, 100), [dict()]),
}
RANGES = ("bench", "three", "runs")         # ... and a candidate range that starts in mid-chunk
_DONE = {}


def _case(name):
    """The case's scans and the oracle's rows, computed once."""
    if name in _DONE:
        return _DONE[name]
    kmin, kmax, w, inc, make, modes = CASES[name]
    rng = np.random.default_rng(4100 + sorted(CASES).index(name))
    seqs = [s.tobytes() for s in make(rng)]
    out = dict(w=w, inc=inc, got=[], part=None)
    with Engine(kmin, kmax) as e:
        e.load(seqs)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        out["fresh"] = e.scan(w, inc)
        for kw in modes:
            res = e.scan(w, inc, chunks=True, **kw)
            out["got"].append((kw, res, e.scan_stat(), e.scan_side()))
        if name in RANGES:
            n = len(out["fresh"])
            out["range"] = (3, n - 2)
            out["part"] = e.scan(w, inc, c0=3, c1=n - 2, chunks=True, **modes[0])
    osym, ometa = OC.genome_profile(seqs, kmin, kmax, False)
    ig = OC.genome_ivom(osym, ometa, kmin, kmax)
    out["exp"] = OC.scan(seqs, ig, kmin, kmax, w, inc, scaffolds_all=False, rip=False)
    _DONE[name] = out
    return out


def _bits(x):
    return x.view(np.uint64 if x.dtype.itemsize == 8 else x.dtype)


def _same_bits(a, b, tag):
    assert len(a) == len(b), tag
    for col in COLS:
        x, y = getattr(a, col), getattr(b, col)
        keep = a.kept if col not in ("seq_index", "start", "stop", "status") else slice(None)
        assert np.array_equal(_bits(x[keep]), _bits(y[keep])), (tag, col)


def _against_oracle(res, exp, tag):
    k = np.nonzero(res.kept)[0]
    assert len(k) == len(exp["kld"]) and len(k) > 0, tag
    assert np.array_equal(res.seq_index[k], exp["seq"]) and np.array_equal(res.start[k], exp["start"]), tag
    assert np.array_equal(res.stop[k], exp["stop"]) and np.array_equal(res.gc[k], exp["gc"], equal_nan=True), tag
    zero = (exp["status"] & OC.ROW_ZERO_DIV) != 0
    assert np.array_equal((res.status[k] & _ffi.ROW_ZERO_WEIGHT) != 0, zero), tag
    ok = ~zero
    worst = float(np.max(np.abs(res.kld[k][ok] - exp["kld"][ok]))) if ok.any() else 0.0
    print("%s: %d kept rows, max |KLD - oracle| = %.3g" % (tag, len(k), worst))
    assert worst <= 1e-11, (tag, worst)
    return len(k)


def _slid_into(res, w, inc):
    """Rows whose window took win_next: not the first of its chunk, a full window one increment behind a full window of the same scaffold."""
    i = np.arange(1, len(res))
    full = (res.stop - res.start + 1) == w
    return (i % CHUNK != 0) & (res.seq_index[i] == res.seq_index[i - 1]) & (res.start[i] == res.start[i - 1] + inc) & full[i] & full[i - 1]


@pytest.mark.parametrize("name", list(CASES))
def test_slid_windows_have_the_fresh_scan_s_bits_and_the_oracle_s_rows(name):
    s = _case(name)
    w, inc, fresh = s["w"], s["inc"], s["fresh"]
    for kw, res, stat, sided in s["got"]:
        tag = "%s (w=%d inc=%d) %s" % (name, w, inc, kw)
        # the narrow-counter kernel ran, in the intended form: 4-bit bulk (plain / side table) where asked for, else 8-bit counters -
        # the 16-bit form (scan_kernel.h, which has no win_step.h in it) reports a width of 16
        want = 4 if kw.get("bits4") or kw.get("side4") else 8
        assert stat[0] == want and sided == bool(kw.get("side4")), (tag, stat, sided)
        _same_bits(fresh, res, tag)
        _against_oracle(res, s["exp"], tag)
    slid = _slid_into(fresh, w, inc)
    assert int(np.count_nonzero(slid)) >= 14, name                  # (most windows of every case are their predecessor moved on)
    starts = fresh.start[1:][slid] - 1                              # 0-based first base of the windows that slid
    its = 20 if w > 2048 else 8
    if name in ("bench", "three", "runs"):
        assert np.all(starts % its == 0)                            # the row-aligned copies only
        assert len(np.unique(starts // (its * 256))) >= 2           # ... and the ring base went round
    if name in ("inc1007", "inc1010", "w2048"):
        assert len(np.unique(starts % its)) >= 2                    # several rows: the general copies, the row's carry
    if name == "runs":
        k4 = s["got"][0]
        assert k4[2][1] >= 1, k4[2]                                 # the poly-A run wrapped a 4-bit counter: windows handed on
        dropped = ~fresh.kept[1:] & slid
        assert int(np.count_nonzero(dropped)) >= 1                  # the N run: windows that slid and were dropped
        assert int(np.count_nonzero(slid[1:] & ~fresh.kept[1:-1])) >= 1     # ... and slid windows behind a dropped one


@pytest.mark.parametrize("name", RANGES)
def test_a_candidate_range_that_starts_in_mid_chunk(name):
    s = _case(name)
    c0, c1 = s["range"]
    assert c0 % CHUNK != 0 and c1 - c0 > 2 * CHUNK          # (the range's chunks count from c0: other windows start a chunk, others slide)
    for col in COLS:
        x, y = getattr(s["part"], col), getattr(s["fresh"], col)[c0:c1]
        assert np.array_equal(_bits(x), _bits(y)), (name, col)
