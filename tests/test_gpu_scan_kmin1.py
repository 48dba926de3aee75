"""The K = 8 4-bit bulk kernels compiled for kmin = 1 (scan8_kernel.h, ROLE bit 2) against the same kernels reading kmin as an
argument (Engine.scan(generic_skeleton=True)), against the scan that counts every window afresh, and against the compiled CPU
oracle: the SAME BITS in every column for the first two, 1e-11 on the KLD (test_gpu_slide.py's bound) for the oracle.

One batch of three scaffolds - 30 kb (26 full windows at w = 5000, inc = 1000: three chunks of 8 and a tail), 20.3 kb and one shorter
than a window - built so that S, the window's count of upper-case A/C/G/T, changes between some consecutive windows and stays
between others: a soft-masked stretch that starts and ends inside a chunk, single Ns, a run of w / 3 Ns that drops windows in
mid-chunk, and a (CA)n run that wraps 4-bit counters in windows of equal S (handed on without the side table)."""
import numpy as np
import pytest

from frisk_amd import _ffi
from frisk_amd.engine import Engine
from oracle import frisk_oracle_c as OC

pytestmark = pytest.mark.gpu

COLS = ("seq_index", "start", "stop", "status", "kld", "gc", "pi", "si", "cri")
GEOMETRIES = ((5000, 1000), (5000, 1007), (2048, 400))
MODES = (dict(bits4=True), dict(side4=True), dict())


def _batch():
    rng = np.random.default_rng(0x51D)
    acgt = np.frombuffer(b"ATGC", dtype=np.uint8)
    a = rng.choice(acgt, size=30000, p=[0.3, 0.3, 0.2, 0.2])
    a[2300:3400] |= 0x20                    # soft-masked: inside the first chunk at every geometry
    a[9500] = ord("N")
    a[13777] = ord("N")
    a[20500:20500 + 5000 // 3 + 1] = ord("N")     # w / 3: the windows that hold all of it are dropped (windows 17..20 of 16..23)
    b = rng.choice(acgt, size=20300, p=[0.2, 0.2, 0.3, 0.3])
    b[6200:6264] = np.resize(np.frombuffer(b"CA", dtype=np.uint8), 64)     # 28 x CACACACA: wraps a 4-bit counter, S unchanged
    b[15001] = ord("N")
    c = rng.choice(acgt, size=1500)
    return [a.tobytes(), b.tobytes(), c.tobytes()]


SEQS = _batch()
_ORACLE = {}


def _bits(x):
    return x.view(np.uint64 if x.dtype.itemsize == 8 else x.dtype)


def _same_bits(a, b, tag, lo=0, hi=None):
    """every column of a equals rows [lo, hi) of b, bit for bit (KLD, GC and the RIP indices where the row is kept)"""
    hi = len(b) if hi is None else hi
    assert len(a) == hi - lo, tag
    for col in COLS:
        x, y = getattr(a, col), getattr(b, col)[lo:hi]
        keep = a.kept if col not in ("seq_index", "start", "stop", "status") else slice(None)
        assert np.array_equal(_bits(x[keep]), _bits(y[keep])), (tag, col)


def _oracle(kmin, w, inc):
    key = (kmin, w, inc)
    if key not in _ORACLE:
        osym, ometa = OC.genome_profile(SEQS, kmin, 8, False)
        ig = OC.genome_ivom(osym, ometa, kmin, 8)
        _ORACLE[key] = OC.scan(SEQS, ig, kmin, 8, w, inc, scaffolds_all=False, rip=kmin <= 2)
    return _ORACLE[key]


def _against_oracle(res, kmin, w, inc, tag):
    exp = _oracle(kmin, w, inc)
    k = np.nonzero(res.kept)[0]
    assert len(k) == len(exp["kld"]) and len(k) > 0, tag
    assert np.array_equal(res.seq_index[k], exp["seq"]) and np.array_equal(res.start[k], exp["start"]), tag
    assert np.array_equal(res.stop[k], exp["stop"]) and np.array_equal(res.gc[k], exp["gc"], equal_nan=True), tag
    zero = (exp["status"] & OC.ROW_ZERO_DIV) != 0
    assert np.array_equal((res.status[k] & _ffi.ROW_ZERO_WEIGHT) != 0, zero), tag
    if kmin <= 2:
        for col in ("pi", "si", "cri"):
            assert np.array_equal(getattr(res, col)[k], exp[col], equal_nan=True), (tag, col)
    ok = ~zero
    worst = float(np.max(np.abs(res.kld[k][ok] - exp["kld"][ok])))
    print("%s: %d rows, max |KLD - oracle| = %.3g" % (tag, len(k), worst))
    assert worst <= 1e-11, (tag, worst)


@pytest.fixture(scope="module")
def engine():
    with Engine(1, 8) as e:
        e.load(SEQS)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        yield e


def test_the_batch_changes_and_keeps_S_and_drops_windows_in_mid_chunk(engine):
    """what the cases below rely on, at the flagship geometry: 26 windows in the first scaffold; consecutive kept windows with
    equal and with different S; dropped windows inside the third chunk; windows handed on by the plain 4-bit form only"""
    r = engine.scan(5000, 1000, bits4=True, chunks=True)
    assert engine.scan_kmin1() and engine.scan_stat()[0] == 4
    handed = engine.scan_stat()[1]
    first = np.nonzero((r.seq_index == 0) & ((r.status & _ffi.ROW_JUMPBACK) == 0))[0]      # (then four jump-back tails)
    assert len(first) == 26 and first[-1] == 25
    kept = r.kept[first]
    assert not kept[17:21].any() and kept[16] and kept[21]
    # (gc holds the fraction here; the rows' S is what the oracle's N counts say: compare neighbours through the sequence itself)
    s = np.frombuffer(SEQS[0], dtype=np.uint8)
    upper = np.isin(s, np.frombuffer(b"ATGC", dtype=np.uint8))
    S = np.array([int(upper[j * 1000:j * 1000 + 5000].sum()) for j in range(26)])
    same = S[1:] == S[:-1]
    assert same.any() and (~same).any() and same[:7].any() and (~same[:7]).any()
    assert handed >= 3
    engine.scan(5000, 1000, side4=True, chunks=True)
    assert engine.scan_kmin1() and engine.scan_side() and engine.scan_stat()[1] == 0


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
def test_specialised_scan_has_the_bits_of_the_generic_and_the_fresh_scan(engine, geom, mode):
    w, inc = GEOMETRIES[geom]
    kw = MODES[mode]
    tag = "w=%d inc=%d %s" % (w, inc, kw)
    fresh = engine.scan(w, inc, rip=True)                    # window by window: every table counted afresh
    assert not engine.scan_kmin1()
    spec = engine.scan(w, inc, rip=True, chunks=True, **kw)
    # (the default starts a short scan at 8 bits: no 4-bit bulk launch, hence none compiled for kmin = 1)
    assert engine.scan_kmin1() == bool(kw) and engine.scan_stat()[0] == (4 if kw else 8), tag
    gen = engine.scan(w, inc, rip=True, chunks=True, generic_skeleton=True, **kw)
    assert not engine.scan_kmin1(), tag
    n = len(fresh)
    assert n > 40 and fresh.kept.sum() > 30, tag
    _same_bits(spec, gen, tag + " generic")
    _same_bits(spec, fresh, tag + " fresh")
    _against_oracle(spec, 1, w, inc, tag)
    # candidate ranges cut at every chunk boundary and one window to either side: a workgroup's first window falls on every
    # kind of window, and whatever a workgroup keeps from window to window starts cold there
    for b in range(8, n, 8):
        for cut in (b - 1, b, b + 1):
            if cut >= n:
                continue
            head = engine.scan(w, inc, rip=True, chunks=True, c0=0, c1=cut, **kw)
            tail = engine.scan(w, inc, rip=True, chunks=True, c0=cut, c1=n, **kw)
            _same_bits(head, spec, tag + " [0, %d)" % cut, 0, cut)
            _same_bits(tail, spec, tag + " [%d, n)" % cut, cut, n)


@pytest.mark.parametrize("kmin", (2, 3))
def test_other_lowest_orders_keep_the_generic_form(kmin):
    with Engine(kmin, 8) as e:
        e.load(SEQS)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        for w, inc in GEOMETRIES:
            for kw in MODES:
                tag = "kmin=%d w=%d inc=%d %s" % (kmin, w, inc, kw)
                r = e.scan(w, inc, rip=kmin <= 2, chunks=True, **kw)
                assert not e.scan_kmin1(), tag
                _against_oracle(r, kmin, w, inc, tag)
