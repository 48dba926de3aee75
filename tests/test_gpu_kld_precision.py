"""The KLD column of every scan form against the extended-precision reference (tests/kld_oracle_hp.py), row by row, within
the per-row bound C_KLD * eps64 * scale that the CPU calibration fixed (tests/test_kld_precision_cpu.py).

The other GPU tests compare KLD with double-precision oracles to a flat 1e-11, which a logarithm 100x worse than the shipped
one passes.  Here every kept, non-zero-weight row of each case (a seeded sample plus every row overlapping an inserted repeat
when a case has more than ~2 000) is held to its own bound, on every kernel route that can score a window, and on the inputs
where FP64 scoring goes wrong: an AT-rich genome scored against GC-rich windows (ratios over many binades), a window that
nearly equals the symmetric profile (KLD ~ 0: the one-pass form T/Sw - ln Sw + ln Sg cancels), windows with N runs and IUPAC
letters, orders with and without interpolation, windows from a query that is not in the profile.  Each case prints its
worst normalised error |KLD - KLD_hp| / (eps64 * scale)."""
import numpy as np
import pytest

import kld_oracle_hp as H

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
WORST = {}


def _bases(rng, n, gc):
    return rng.choice(ACGT, size=n, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])


def _revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def _genome(seed, lens, gc=0.15, islands=0, island_len=3000, orphans=0, repeats=0, units=(b"A", b"CA"), rep_lens=(20, 60, 200)):
    """Scaffolds of an AT-rich genome (GC fraction `gc`) with GC-rich islands (GC 0.75), orphans (N runs of 1-40 bases and IUPAC
    letters) and simple repeats, all at seeded places.  Returns (list of bytes, per scaffold list of repeat intervals)."""
    rng = np.random.default_rng(seed)
    seqs, reps = [], []
    for n in lens:
        s = _bases(rng, n, gc)
        for _ in range(islands):
            a = int(rng.integers(0, max(1, n - island_len)))
            s[a:a + island_len] = _bases(rng, len(s[a:a + island_len]), 0.75)
        for _ in range(orphans):
            a = int(rng.integers(0, n))
            ln = int(rng.integers(1, 41))
            s[a:a + ln] = ord("N") if rng.integers(0, 2) else rng.choice(np.frombuffer(b"RYKMSW", np.uint8), size=len(s[a:a + ln]))
        iv = []
        for _ in range(repeats):
            u = units[int(rng.integers(0, len(units)))]
            ln = int(rng.choice(rep_lens))
            a = int(rng.integers(0, max(1, n - ln)))
            s[a:a + ln] = np.frombuffer((u * (ln // len(u) + 1))[:ln], np.uint8)
            iv.append((a, a + ln))
        seqs.append(s.tobytes())
        reps.append(iv)
    return seqs, reps


def _engine(kmin, kmax, seqs, prof):
    from frisk_amd.engine import Engine
    e = Engine(kmin, kmax)
    e.load(seqs)
    sym, meta = prof
    e.profile_set(sym, *[int(v) for v in meta])
    return e


def _check(tag, res, seqs, prof, kmin, kmax, w, inc, scaffolds_all=False, reps=None, sample=2000, seed=0):
    """Every kept row of `res` (a frisk_scan result) against the reference within its bound; rows sampled (plus every row that
    overlaps a repeat) when there are more than `sample` candidates.  Returns the worst normalised error."""
    from frisk_amd import _ffi
    allc = H.candidates(seqs, w, inc, scaffolds_all)
    assert res.n_candidates == len(allc), tag
    if len(allc) <= sample:
        sel = None
    else:
        rng = np.random.default_rng(seed)
        sel = set(rng.choice(len(allc), size=sample * 3 // 4, replace=False).tolist())
        if reps:
            over = [k for k, si, a, b, _, _ in allc if any(x < b and y > a for x, y in reps[si])]
            sel |= set(rng.permutation(over)[:sample // 2].tolist())
    r = H.scan_hp(seqs, prof, kmin, kmax, w, inc, scaffolds_all, cand=sel)
    k = r["cand"]
    if sel is None:
        assert np.array_equal(np.nonzero(res.kept)[0], k), tag
    assert res.kept[k].all(), tag
    assert np.array_equal(res.start[k], r["start"]) and np.array_equal(res.stop[k], r["stop"]), tag
    zero = (res.status[k] & _ffi.ROW_ZERO_WEIGHT) != 0
    assert np.array_equal(zero, r["flag"] == H.ZERO_DIV), tag
    assert np.array_equal((res.status[k] & _ffi.ROW_NO_MAXMER) != 0, r["flag"] == H.NO_MAXMER), tag
    ok = r["flag"] == H.OK
    assert ok.sum() >= min(20, len(k)), (tag, int(ok.sum()))
    got = res.kld[k][ok]
    err = np.abs(got.astype(np.longdouble) - r["kld_hp"][ok])
    norm = H.normalised_error(got, r["kld_hp"][ok], r["scale"][ok])
    worst = float(norm.max())
    j = int(np.argmax(norm))
    print("%-52s rows %5d  worst normalised error %6.2f  (|dKLD| %.2e at KLD %.3g)" % (
        tag, int(ok.sum()), worst, float(err[j]), float(r["kld"][ok][j])))
    WORST[tag] = max(WORST.get(tag, 0.0), worst)
    bad = np.nonzero(err > H.bound(r["scale"][ok]))[0]
    assert not bad.size, "%s: %d rows over the bound; worst normalised error %.1f (C_KLD = %g) at candidate %d" % (
        tag, bad.size, worst, H.C_KLD, int(k[ok][j]))
    return worst


@pytest.fixture(scope="module")
def skewed():
    """An 85 % AT genome (the profile) with a few GC-rich islands, N runs and IUPAC letters, plus a GC-rich query."""
    seqs, _ = _genome(1, [400_000, 150_000, 7_000], gc=0.15, islands=12, orphans=60)
    query, _ = _genome(2, [60_000, 25_000], gc=0.62, islands=4, orphans=20)
    return seqs, query


@pytest.mark.parametrize("w,inc", [(2000, 500), (2000, 1500), (5000, 1000), (5000, 4000)])
@pytest.mark.parametrize("form", ["bits4", "side4"])
def test_scan8_four_bit_forms(skewed, form, w, inc):
    """scan8_kernel.h, K = 8, 4-bit counters (plain and with the side table), both window classes (ITS 8 / 20), tables sliding
    (2 inc <= w - 7) or not; the windows of the AT-rich genome itself and of the GC-rich query against its profile."""
    seqs, query = skewed
    prof = H.profile(seqs, 1, 8)
    for name, win in (("genome", seqs), ("query", query)):
        with _engine(1, 8, win, prof) as e:
            res = e.scan(w, inc, **{form: True})
            assert e.scan_stat()[0] == 4 and e.scan_side() == (form == "side4"), e.scan_stat()
        _check("scan8 4-bit %s w=%d i=%d %s" % (form, w, inc, name), res, win, prof, 1, 8, w, inc)


@pytest.mark.parametrize("w,inc", [(2000, 700), (5000, 2500)])
def test_scan8_eight_bit_bulk_with_dense_repeats(w, inc):
    """A short scan (too few windows to sample a width: 8-bit bulk) over a genome dense with poly-A and (CA)n runs of 20-200
    bases: max-mers occurring 16+ times take the reciprocal + Newton path of the 8-bit form."""
    seqs, reps = _genome(3, [500_000], gc=0.4, orphans=30, repeats=500)
    prof = H.profile(seqs, 1, 8)
    with _engine(1, 8, seqs, prof) as e:
        res = e.scan(w, inc)
        assert e.scan_stat()[0] == 8, e.scan_stat()
    _check("scan8 8-bit bulk w=%d i=%d" % (w, inc), res, seqs, prof, 1, 8, w, inc, reps=reps)


def test_scan8_handover_four_eight_sixteen():
    """Runs of 300-900 bases make max-mers that occur 256+ times in a window: the 4-bit form hands those windows to the 8-bit
    form and that one on to the 16-bit form (scan_kernel.h)."""
    seqs, reps = _genome(4, [700_000], gc=0.3, repeats=120, units=(b"A", b"CA", b"GATA"), rep_lens=(24, 150, 320, 600, 900))
    prof = H.profile(seqs, 1, 8)
    with _engine(1, 8, seqs, prof) as e:
        res = e.scan(5000, 1000, bits4=True)
        st = e.scan_stat()
    assert st[0] == 4 and st[1] > 0 and st[2] > 0, st
    _check("scan8 hand-over 4->8->16 w=5000 i=1000", res, seqs, prof, 1, 8, 5000, 1000, reps=reps)


@pytest.mark.parametrize("kmax", [6, 7])
@pytest.mark.parametrize("kmin,w,inc", [(1, 2000, 500), (2, 5000, 3000)])
def test_scan8_orders_six_and_seven(skewed, kmax, kmin, w, inc):
    seqs, query = skewed
    prof = H.profile(seqs, kmin, kmax)
    for name, win in (("genome", seqs), ("query", query)):
        with _engine(kmin, kmax, win, prof) as e:
            res = e.scan(w, inc)
        _check("scan8 K=%d kmin=%d w=%d i=%d %s" % (kmax, kmin, w, inc, name), res, win, prof, kmin, kmax, w, inc)


@pytest.mark.parametrize("kmin,kmax,w,inc", [
    (6, 8, 2000, 600), (8, 8, 3000, 1000),                    # K8 form of scan_kernel.h: kmin above the shared prefix level
    (1, 8, 6000, 1500), (1, 8, 12000, 5000), (6, 8, 40000, 15000),    # ITS 16; 1024-thread runtime loops
    (1, 4, 2000, 500), (5, 5, 1000, 400), (7, 7, 2000, 900), (5, 6, 3000, 1000)])     # the other forms
def test_scan_kernel_sixteen_bit_forms(skewed, kmin, kmax, w, inc):
    seqs, query = skewed
    prof = H.profile(seqs, kmin, kmax)
    # (a GC-rich query against an AT-rich genome: with kmin > 3 nearly every window holds a max-mer the genome lacks - zero weight)
    for name, win in (("genome", seqs), ("query", query))[:2 if kmin <= 3 else 1]:
        with _engine(kmin, kmax, win, prof) as e:
            res = e.scan(w, inc)
            assert e.scan_stat()[0] == 16, e.scan_stat()
        _check("scan_kernel K=%d kmin=%d w=%d i=%d %s" % (kmax, kmin, w, inc, name), res, win, prof, kmin, kmax, w, inc)


@pytest.mark.parametrize("kmin,kmax,w,inc,lens", [
    (1, 8, 70000, 20000, [300_000]),                          # windows beyond the 16-bit LDS counters
    (1, 10, 3000, 1400, [60_000, 9_000]),                     # K > 8: global-memory tables
    (12, 12, 20000, 9000, [90_000])])
def test_scan_big_kernel(kmin, kmax, w, inc, lens):
    seqs, _ = _genome(5, lens, gc=0.2, islands=6, island_len=8000, orphans=20)
    prof = H.profile(seqs, kmin, kmax)
    with _engine(kmin, kmax, seqs, prof) as e:
        res = e.scan(w, inc)
    _check("scan_big K=%d kmin=%d w=%d i=%d" % (kmax, kmin, w, inc), res, seqs, prof, kmin, kmax, w, inc)


@pytest.mark.parametrize("kmin,kmax,w", [(1, 8, 5000), (1, 6, 5000), (1, 4, 3000), (8, 8, 8000)])
def test_window_equal_to_the_symmetric_profile(kmin, kmax, w):
    """A scaffold s + revcomp(s), scanned whole (scaffoldsAll), in a genome that holds it and a 400-base scaffold besides: the
    window's counts are half the genome's symmetric counts but for the small scaffold's, pw ~ pg and the KLD is tiny, so T/Sw,
    ln Sw and ln Sg cancel almost completely.  (Without the second scaffold pw = pg exactly and every form returns 0.)"""
    rng = np.random.default_rng(6)
    s = _bases(rng, int(w * 0.6), 0.3).tobytes()
    seqs = [s + _revcomp(s), _bases(rng, 400, 0.5).tobytes()]
    prof = H.profile(seqs, kmin, kmax)
    with _engine(kmin, kmax, seqs, prof) as e:
        res = e.scan(w, w // 4, scaffolds_all=True)
    assert res.n_candidates == 2
    _check("near-zero KLD K=%d kmin=%d whole scaffold" % (kmax, kmin), res, seqs, prof, kmin, kmax, w, w // 4, scaffolds_all=True)
    assert 0 < abs(res.kld[0]) < 1e-2, res.kld[0]


def test_two_row_segments():
    """More than 2^17 candidates: the last sixteenth of the scan runs as a second launch (scan_stat()[3] == 2).  Sampled rows,
    rows overlapping the repeats and the rows around the cut."""
    seqs, reps = _genome(7, [12_000_000], gc=0.4, orphans=400, repeats=200, units=(b"A", b"CA", b"AAT", b"TTAGGG"),
                         rep_lens=(40, 150, 400))
    prof = H.profile(seqs, 1, 8)
    w, inc = 5000, 90
    with _engine(1, 8, seqs, prof) as e:
        res = e.scan(w, inc)
        st = e.scan_stat()
    n = res.n_candidates
    assert n > (1 << 17) and st[3] == 2, (n, st)
    _check("two row segments w=%d i=%d" % (w, inc), res, seqs, prof, 1, 8, w, inc, reps=reps, sample=1600)
    unit = 16 * 16
    cut = (n // unit - max(1, n // unit // 16)) * unit
    sub = H.scan_hp(seqs, prof, 1, 8, w, inc, cand=(cut - 150, cut + 150))
    ok = sub["flag"] == H.OK
    err = np.abs(res.kld[sub["cand"]][ok] - sub["kld"][ok])
    assert (err <= H.bound(sub["scale"][ok])).all()


@pytest.mark.parametrize("kmin,kmax,w,inc", [(1, 4, 2000, 700), (1, 6, 3000, 1000), (5, 6, 2000, 900), (3, 3, 1000, 500)])
def test_ivom_vectors(skewed, kmin, kmax, w, inc):
    """frisk_scan_ivom's normalised window and genome distributions per entry against the long-double pw, pg:
    |gpu - hp| <= C_IVOM (K + 2) eps64 hp, for the genome's windows and the query's."""
    seqs, query = skewed
    prof = H.profile(seqs, kmin, kmax)
    for name, win in (("genome", seqs[1:]), ("query", query))[:2 if kmin <= 3 else 1]:
        with _engine(kmin, kmax, win, prof) as e:
            e.scan(w, inc)
            wi, gi = e.scan_ivom(w, inc)
        r = H.scan_hp(win, prof, kmin, kmax, w, inc, keep_ivom=True)
        worst, rows = 0.0, 0
        for t, k in enumerate(r["cand"]):
            if r["flag"][t] != H.OK:
                continue
            present, pw, pg = r["ivom"][t]
            worst = max(worst, H.ivom_error(wi[k], present, pw, kmax), H.ivom_error(gi[k], present, pg, kmax))
            rows += 1
        print("IVOM K=%d kmin=%d %s: %d rows, worst error %.2f (K + 2) eps64 (C_IVOM = %g)" % (kmax, kmin, name, rows, worst, H.C_IVOM))
        assert rows >= 20 and worst <= H.C_IVOM, (name, worst)


def test_zz_report():
    """(runs last) the worst normalised error per case, in one table."""
    for tag, v in sorted(WORST.items()):
        print("%-52s %6.2f" % (tag, v))
    assert max(WORST.values(), default=0.0) <= H.C_KLD
