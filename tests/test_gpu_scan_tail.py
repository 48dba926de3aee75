"""The K = 8 scoring loop in two halves per position (scan8_kernel.h: score_front, score_back - the 4-bit form's loop in groups of
two runs a group's back halves, which need the logarithm table's entry, behind the next group's front halves), and the per-window
work around it: a slid window's table updates, the wave sums and totals behind the loop, the clearing of the small tables.  How a
position's operations are spread over the loop, and which form scored a window, must not show in a row: every column of the chunked
scan (Engine.scan(chunks=True): tables slide inside a chunk) has the bits of the scan that counts every window afresh, in the 4-bit
form (halves), the 4-bit form with the side table and the 8-bit form (whole positions) alike, and the rows agree with the C oracle to
1e-11 (test_gpu_slide.py's bound; the window-by-window scan runs the same loop - what makes the reference independent of it is the
oracle).

K = 8, kmin = 1.  A batch: a scaffold of 45 kb with a run of 40 invalid bases across the boundary of two leaving ranges, one across
the boundary of two entering ranges, a run of w / 3 (windows dropped in mid-chunk), single invalid bases and a soft-masked stretch; a
scaffold of 30 kb with a (CA)n run (the side table's business; wraps a 4-bit counter); a scaffold shorter than a window.  Geometries
(w, inc) - every copy of the loop and every path of a slid window's table updates (positions of the leaving and entering range per thread):
  * (5000, 1000): the flagship, 4 positions per thread, threads 250 .. 255 without one - the row-aligned copies of the scoring loop;
  * (5000, 1007): the general copies;
  * (5000, 1): one position, one live thread (a range of 300 candidates around the invalid runs: no oracle for this one);
  * (5000, 255), (5000, 256), (5000, 257): one position per thread, every thread live, two positions with a last live thread that holds one;
  * (5000, 1024): every slot live;
  * (5000, 2496): the largest increment that slides, 10 positions per thread;
  * (2048, 400): the instantiation with 8 positions per lane (halves too: groups of two);
  * (5000, 1000) with the RIP columns, which read the small tables just in front of the scoring loop, and whole-scaffold windows."""
import numpy as np
import pytest

from frisk_amd import _ffi
from frisk_amd.engine import Engine
from oracle import frisk_oracle_c as OC

pytestmark = pytest.mark.gpu

COLS = ("seq_index", "start", "stop", "status", "kld", "gc")
RIP_COLS = ("pi", "si", "cri")
CHUNK = 8                                   # windows per chunk of a scan with chunks=True (scan_schedule.h)
K = 8
ACGT = np.frombuffer(b"ATGC", dtype=np.uint8)
MODES = (dict(bits4=True), dict(side4=True), dict())


def _batch(rng, w, inc):
    a = rng.choice(ACGT, size=45000, p=[0.3, 0.3, 0.2, 0.2])
    lo = max(7 * inc - 20, 700)
    a[lo:lo + 40] = ord("N")                            # across the boundary of two leaving ranges (window starts are multiples of inc)
    hi = max(12 * inc, 800) + w - (K - 1) - 20
    a[hi:hi + 40] = ord("N")                            # ... of two entering ranges (inc positions before a window's last K - 1)
    for p in (3, 997, 2 * inc + 5, 20011, 20012 + K):   # single invalid bases: short words, orphans
        a[p] = ord("N")
    a[30000:30000 + w // 3] = ord("N")                  # 30 % of a window and more: windows dropped in mid-chunk
    a[9000:11500] |= 0x20                               # soft-masked
    b = rng.choice(ACGT, size=30000, p=[0.25, 0.25, 0.25, 0.25])
    b[14000:14060] = np.resize(np.frombuffer(b"CA", dtype=np.uint8), 60)
    b[22000:22003] = ord("n")
    c = rng.choice(ACGT, size=w - 1000, p=[0.25, 0.25, 0.25, 0.25])
    return [a.tobytes(), b.tobytes(), c.tobytes()]


# name: (w, inc, scan arguments, candidate range or None)
CASES = {
    "flagship": (5000, 1000, dict(), None),
    "inc1007":  (5000, 1007, dict(), None),
    "inc1":     (5000, 1, dict(), (600, 900)),          # windows 600 .. 899 of the first scaffold: both runs of 40 pass through both ranges
    "inc255":   (5000, 255, dict(), None),
    "inc256":   (5000, 256, dict(), None),
    "inc257":   (5000, 257, dict(), None),
    "inc1024":  (5000, 1024, dict(), None),
    "inc2496":  (5000, 2496, dict(), None),
    "w2048":    (2048, 400, dict(), None),
    "rip":      (5000, 1000, dict(rip=True, scaffolds_all=True), None),
}
_DONE = {}


def _case(name):
    """The case's scans, computed once."""
    if name in _DONE:
        return _DONE[name]
    w, inc, kw, rng_ = CASES[name]
    rng = np.random.default_rng(5200 + sorted(CASES).index(name))
    seqs = _batch(rng, w, inc)
    span = dict(c0=rng_[0], c1=rng_[1]) if rng_ else {}
    out = dict(w=w, inc=inc, kw=kw, seqs=seqs, got=[])
    with Engine(1, K) as e:
        e.load(seqs)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        out["fresh"] = e.scan(w, inc, **kw, **span)
        for mode in MODES:
            res = e.scan(w, inc, chunks=True, **kw, **span, **mode)
            out["got"].append((mode, res, e.scan_stat(), e.scan_side()))
    _DONE[name] = out
    return out


def _bits(x):
    return x.view(np.uint64 if x.dtype.itemsize == 8 else x.dtype)


def _same_bits(a, b, cols, tag):
    assert len(a) == len(b) and len(a) > 0, tag
    for col in cols:
        x, y = getattr(a, col), getattr(b, col)
        keep = a.kept if col not in ("seq_index", "start", "stop", "status") else slice(None)
        assert np.array_equal(_bits(x[keep]), _bits(y[keep])), (tag, col)


def _slid_into(res, w, inc):
    """Rows whose window slid: not the first of its chunk, a full window one increment behind a full window of the same scaffold."""
    i = np.arange(1, len(res))
    full = (res.stop - res.start + 1) == w
    return (i % CHUNK != 0) & (res.seq_index[i] == res.seq_index[i - 1]) & (res.start[i] == res.start[i - 1] + inc) & full[i] & full[i - 1]


@pytest.mark.parametrize("name", list(CASES))
def test_chunked_scans_have_the_fresh_scan_s_bits_in_every_form(name):
    s = _case(name)
    w, inc, fresh = s["w"], s["inc"], s["fresh"]
    cols = COLS + (RIP_COLS if s["kw"].get("rip") else ())
    assert len(fresh) <= 400, (name, len(fresh))
    for mode, res, stat, sided in s["got"]:
        tag = "%s (w=%d inc=%d) %s" % (name, w, inc, mode)
        want = 4 if mode.get("bits4") or mode.get("side4") else 8
        assert stat[0] == want and sided == bool(mode.get("side4")), (tag, stat, sided)
        _same_bits(fresh, res, cols, tag)
    for i in range(len(MODES)):
        for j in range(i + 1, len(MODES)):
            _same_bits(s["got"][i][1], s["got"][j][1], cols, "%s: %s against %s" % (name, MODES[i], MODES[j]))
    slid = _slid_into(fresh, w, inc)
    assert int(np.count_nonzero(slid)) >= (20 if inc < 2000 else 12), name
    assert int(np.count_nonzero(slid & ~fresh.kept[1:])) >= 1 or name == "inc1", name        # a window that slid and was dropped (the long N run)
    plain, side = s["got"][0], s["got"][1]
    if name != "inc1":
        assert plain[2][1] >= 1, (name, plain[2])               # the (CA)n run wrapped a 4-bit counter: windows handed on ...
        assert side[2][1] < plain[2][1], (name, side[2])        # ... which the side table kept
    its = 20 if w > 2048 else 8
    starts = fresh.start[1:][slid] - 1
    if name in ("flagship", "rip"):
        assert np.all(starts % its == 0)                        # the row-aligned copies only
    if name in ("inc1007", "inc257", "inc1"):
        assert len(np.unique(starts % its)) >= 2                # the general copies


@pytest.mark.parametrize("name", [n for n in CASES if n != "inc1"])
def test_the_rows_are_the_oracle_s(name):
    s = _case(name)
    w, inc, kw, seqs = s["w"], s["inc"], s["kw"], s["seqs"]
    osym, ometa = OC.genome_profile(seqs, 1, K, False)
    ig = OC.genome_ivom(osym, ometa, 1, K)
    exp = OC.scan(seqs, ig, 1, K, w, inc, scaffolds_all=bool(kw.get("scaffolds_all")), rip=bool(kw.get("rip")))
    for mode, res, _, _ in [(None, s["fresh"], None, None)] + s["got"]:
        tag = "%s (w=%d inc=%d) %s" % (name, w, inc, mode)
        k = np.nonzero(res.kept)[0]
        assert len(k) == len(exp["kld"]) and len(k) > 0, tag
        assert np.array_equal(res.seq_index[k], exp["seq"]) and np.array_equal(res.start[k], exp["start"]), tag
        assert np.array_equal(res.stop[k], exp["stop"]) and np.array_equal(res.gc[k], exp["gc"], equal_nan=True), tag
        zero = (exp["status"] & OC.ROW_ZERO_DIV) != 0
        assert np.array_equal((res.status[k] & _ffi.ROW_ZERO_WEIGHT) != 0, zero), tag
        if kw.get("rip"):
            for col in RIP_COLS:
                assert np.array_equal(getattr(res, col)[k], exp[col], equal_nan=True), (tag, col)
        ok = ~zero
        worst = float(np.max(np.abs(res.kld[k][ok] - exp["kld"][ok])))
        print("%s: %d kept rows, max |KLD - oracle| = %.3g" % (tag, len(k), worst))
        assert worst <= 1e-11, (tag, worst)
