"""The two forms of the ring access in the K = 8 scoring loop (scan8_kernel.h, frisk_amd/csrc/ring_rows.h): a window whose first base
sits on row 0 of the ring (rb_r = st % ITS = 0) takes the row-aligned copies, every other window the general ones.  Which form a
window takes must not show in its row: the same lanes read the same values and add them in the same order.

K = 8, kmin = 1, w = 3000 (ITS = 20, the ring is on), one engine per increment:
  * inc = 600: rb_r = 0 for every window that slides - the row-aligned copies only;
  * inc = 610: rb_r alternates between 0 and 10 - both forms inside one chunk, the ring handed from one to the other;
  * inc = 607: the general form only (the control);
and the benchmark's own geometry, w = 5000 and inc = 1000, on one 40 kb scaffold.
Each scan with sliding tables and the ring (chunks=True, 4-bit bulk and 4-bit + side table) must give the bits of the scan that
counts every window afresh and gathers every value from the table, and the C oracle's rows to 1e-11 (test_gpu_slide.py's bound)."""
import numpy as np
import pytest

from frisk_amd import _ffi
from frisk_amd.engine import Engine
from oracle import frisk_oracle_c as OC

pytestmark = pytest.mark.gpu

COLS = ("seq_index", "start", "stop", "status", "kld", "gc")
KMIN, KMAX = 1, 8
CHUNK = 8                                   # windows per chunk of a scan with chunks=True (scan_schedule.h)
CASES = {"inc600": (3000, 600), "inc610": (3000, 610), "inc607": (3000, 607), "bench": (5000, 1000)}
ACGT = np.frombuffer(b"ATGC", dtype=np.uint8)


def _seqs(w, inc, seed):
    rng = np.random.default_rng(seed)
    draw = lambda n: rng.choice(ACGT, size=n, p=[0.3, 0.3, 0.2, 0.2])      # noqa: E731
    if w == 5000:
        return [draw(40000).tobytes()]
    a = draw(20000)                         # more than 3 x 5120 positions: the ring's columns wrap
    b = draw(12000)                         # a short N run and a soft-masked stretch: the copies without ALLON
    b[4000:4040] = ord("N")
    b[7000:7900] |= 0x20
    c = draw(15000)                         # a dropped window in mid-chunk: its successor gathers afresh
    c[5 * inc:5 * inc + w] = ord("N")
    d = draw(9 * inc + w + 17)              # a jumpback tail
    return [a.tobytes(), b.tobytes(), c.tobytes(), d.tobytes()]


@pytest.fixture(scope="module")
def scans():
    """Every case's three scans and the oracle's rows, computed once."""
    out = {}
    for no, (name, (w, inc)) in enumerate(CASES.items()):
        seqs = _seqs(w, inc, 9100 + no)
        with Engine(KMIN, KMAX) as e:
            e.load(seqs)
            e.profile_reset(); e.profile_add(); e.profile_finalize()
            fresh = e.scan(w, inc)
            bits4 = e.scan(w, inc, chunks=True, bits4=True)
            width4 = e.scan_stat()[0]
            side4 = e.scan(w, inc, chunks=True, side4=True)
            width_side, sided = e.scan_stat()[0], e.scan_side()
        osym, ometa = OC.genome_profile(seqs, KMIN, KMAX, False)
        ig = OC.genome_ivom(osym, ometa, KMIN, KMAX)
        exp = OC.scan(seqs, ig, KMIN, KMAX, w, inc, scaffolds_all=False, rip=False)
        out[name] = dict(w=w, inc=inc, fresh=fresh, bits4=bits4, side4=side4, exp=exp, width4=width4, width_side=width_side, sided=sided)
    return out


def _same_bits(a, b, tag):
    assert len(a) == len(b), tag
    for col in COLS:
        x, y = getattr(a, col), getattr(b, col)
        keep = a.kept if col not in ("seq_index", "start", "stop", "status") else slice(None)
        assert np.array_equal(x[keep].view(np.uint64 if x.dtype.itemsize == 8 else x.dtype),
                              y[keep].view(np.uint64 if y.dtype.itemsize == 8 else y.dtype)), (tag, col)


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
    """Kept rows whose window slid into its predecessor's table: not the first of its chunk, behind a kept full window of the
    same scaffold one increment before it (a dropped predecessor leaves no ring: its successor gathers afresh), itself a full window."""
    i = np.arange(1, len(res))
    full = (res.stop - res.start + 1) == w
    slid = (i % CHUNK != 0) & (res.seq_index[i] == res.seq_index[i - 1]) & (res.start[i] == res.start[i - 1] + inc) & full[i] & full[i - 1]
    return int(np.count_nonzero(slid & res.kept[i] & res.kept[i - 1]))


def _check(s, name):
    tag = "%s (w=%d inc=%d)" % (name, s["w"], s["inc"])
    assert s["width4"] == 4 and s["width_side"] == 4 and s["sided"], tag
    _same_bits(s["fresh"], s["bits4"], tag + " 4-bit bulk")
    _same_bits(s["fresh"], s["side4"], tag + " 4-bit bulk + side table")
    n = _against_oracle(s["bits4"], s["exp"], tag + " 4-bit bulk")
    assert _against_oracle(s["side4"], s["exp"], tag + " 4-bit bulk + side table") == n
    slid = _slid_into(s["bits4"], s["w"], s["inc"])
    assert slid >= 1, tag
    return n


@pytest.mark.parametrize("name", list(CASES))
def test_ring_forms_give_the_fresh_scan_s_bits_and_the_oracle_s_rows(scans, name):
    s = scans[name]
    _check(s, name)
    r = s["bits4"]
    full = r.kept & ((r.stop - r.start + 1) == s["w"])       # (a jumpback window reports a 0-based start: w + 1)
    starts = r.start[full] - 1                               # 0-based first base of the kept full windows
    rows0 = int(np.count_nonzero(starts % 20 == 0))
    assert len(starts) > 20
    if name in ("inc600", "bench"):
        assert rows0 == len(starts)                          # (every full window: the row-aligned copies)
    elif name == "inc610":
        assert 0.3 * len(starts) < rows0 < 0.7 * len(starts) # (both forms, alternating)
    else:
        assert rows0 <= len(starts) // 10 + 1                # (one start in twenty sits on row 0)


def test_more_than_a_hundred_rows_were_compared(scans):
    assert sum(int(np.count_nonzero(s["bits4"].kept)) for s in scans.values()) > 100
