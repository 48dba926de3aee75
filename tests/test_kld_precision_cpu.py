"""The extended-precision KLD reference (tests/kld_oracle_hp.py) and its per-row bound, without a GPU.

  * the reference is itself high precision: it agrees with a 40-digit mpmath evaluation from the golden integer counts;
  * calibration: C_KLD is the smallest power of two that is at least four times the worst normalised error of three
    double implementations on every golden row (the reference's own KLDs, oracle/frisk_oracle_np.py, the compiled C
    oracle), and all three lie within the bound; C_IVOM likewise for the normalised IVOM vectors.  The C oracle on cases of
    the GPU fuzz generator is checked too, with an allowance for its sequentially summed Sw, Sg (see that test);
  * the bound is sharp enough to matter: a numpy emulation of scan8_kernel.h's table logarithm (log_tab_n: 64 bins,
    degree-6 Taylor polynomial of log1p, the table frisk_abi.hip builds) scored with the one-pass form stays inside it,
    and the same emulation with a degree-4 polynomial, or with the bin index one too high, falls outside it.
"""
import functools
import math

import numpy as np
import pytest

import kld_oracle_hp as H
from fuzz_cases import random_case
from golden_util import Case, case_names
from oracle import frisk_oracle_c as OC
from oracle import frisk_oracle_np as N

LD = np.longdouble


def _golden_inputs(c):
    host = H.read_fasta(c.host)
    return host, (H.read_fasta(c.query) if c.query else host)


@functools.lru_cache(maxsize=None)
def _golden_hp(name):
    c = Case(name)
    host, q = _golden_inputs(c)
    prof = H.profile(host, c.m, c.k, c.mask_host)
    r = H.scan_hp(q, prof, c.m, c.k, c.w, c.i, c.scaffolds_all, keep_ivom=True)
    assert len(r["cand"]) == len(c.rows)
    assert np.array_equal(r["flag"] == H.ZERO_DIV, np.array(["error" in row for row in c.rows]))
    return c, host, q, prof, r


def _worst(kld, r, ok):
    return float(np.max(H.normalised_error(kld[ok], r["kld_hp"][ok], r["scale"][ok]))) if ok.any() else 0.0


def test_window_counts_are_the_oracle_counts():
    """The sparse per-window counting of the reference (only the max-mers present, their prefixes gathered per order) gives
    the dense forward counts of N.forward_counts, including windows with N runs and soft-masked bases."""
    rng = np.random.default_rng(5)
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3000)
    s[100:140] = ord("N"); s[700:760] |= 0x20; s[2000:2003] = ord("R")
    enc = N.Encoded(s.tobytes())
    for kmin, kmax in ((1, 8), (3, 5), (6, 6)):
        present, cs, S = H.window_counts(enc, kmin, kmax)
        dense, _ = N.forward_counts(enc, kmin, kmax)
        assert np.array_equal(present, np.nonzero(dense[N.table_offset(kmin, kmax):])[0])
        for t, c in enumerate(cs):
            x = kmin + t
            assert np.array_equal(c, dense[N.table_offset(kmin, x) + (present >> (2 * (kmax - x)))])
        assert S == int(enc.upper.sum())


def _kld_mpmath(wcounts, S, gcounts, meta, kmin, kmax):
    """The reference's KLD at 40 digits from dense count tables: IVOM recursion, sums and logarithms all in mpmath."""
    import mpmath as mp
    mp.mp.dps = 40
    top = wcounts[N.table_offset(kmin, kmax):]
    present = np.nonzero(top)[0]

    def ivom(counts, space):
        W, I = 0, [mp.mpf(0)] * present.size
        Ws = [0] * present.size
        for x in range(kmin, kmax + 1):
            cx = counts[N.table_offset(kmin, x) + (present >> (2 * (kmax - x)))]
            D = (space - (x - 1)) * 2
            for j in range(present.size):
                c = int(cx[j])
                wt = c * 4 ** x
                Ws[j] += wt
                a = mp.mpf(wt) / Ws[j]
                p = mp.mpf(c) / D
                I[j] = a * p if x == kmin else a * p + (1 - a) * I[j]
        return I
    Iw = ivom(wcounts, S)
    Ig = ivom(gcounts, int(meta[0]) - int(meta[2]))
    Sw, Sg = mp.fsum(Iw), mp.fsum(Ig)
    return mp.fsum((a / Sw) * mp.log((a / Sw) / (b / Sg)) for a, b in zip(Iw, Ig)) / mp.log(2)


def test_reference_agrees_with_mpmath():
    """~20 golden rows, drawn with a fixed seed: kld_hp (computed from the sequences) against a 40-digit evaluation from the
    golden count tables (the reference's own computeKmers output) to 1e-17 * scale."""
    import mpmath as mp
    rng = np.random.default_rng(11)
    picks = []
    for name in case_names():
        c = Case(name)
        ok = [t for t, row in enumerate(c.rows) if "error" not in row and row.get("KLD", 0) != 0]
        picks += [(name, t) for t in rng.permutation(ok)[:2]]
    picks = [picks[i] for i in sorted(rng.choice(len(picks), size=min(20, len(picks)), replace=False))]
    worst = 0.0
    for name, t in picks:
        c, host, q, prof, r = _golden_hp(name)
        row = c.rows[t]
        S = row["meta"][0] - row["meta"][2]
        want = _kld_mpmath(c.window_counts[t].astype(np.int64), S, c.genome_counts.astype(np.int64), c.genome_meta, c.m, c.k)
        hi = float(r["kld_hp"][t])
        err = abs(mp.mpf(hi) + mp.mpf(float(r["kld_hp"][t] - LD(hi))) - want)        # (the long double, exactly)
        worst = max(worst, float(err / r["scale"][t]))
        assert err <= 1e-17 * r["scale"][t], (name, t, float(err))
    print("long double reference vs mpmath on %d golden rows: worst |error| / scale = %.3g" % (len(picks), worst))
    assert len(picks) >= 15


@functools.lru_cache(maxsize=None)
def _calibration():
    """Worst normalised error of each double implementation (and the number of rows it was measured on)."""
    out = {}
    # 1. the reference's own KLDs, every golden case (query-file cases included)
    worst, n = 0.0, 0
    for name in case_names():
        c, host, q, prof, r = _golden_hp(name)
        ok = r["flag"] == H.OK
        gold = np.array([row.get("KLD", np.nan) if "error" not in row else np.nan for row in c.rows])
        worst, n = max(worst, _worst(gold, r, ok)), n + int(ok.sum())
    out["golden"] = (worst, n)
    # 2. the numpy oracle, every golden case
    worst, n = 0.0, 0
    for name in case_names():
        c, host, q, prof, r = _golden_hp(name)
        rows = N.scan(list(enumerate(q)), prof, c.m, c.k, c.w, c.i, c.scaffolds_all)
        assert len(rows) == len(r["cand"])
        ok = r["flag"] == H.OK
        kld = np.array([row.get("KLD", np.nan) for row in rows], dtype=np.float64)
        worst, n = max(worst, _worst(kld, r, ok)), n + int(ok.sum())
    out["numpy oracle"] = (worst, n)
    # 3. the compiled C oracle, every golden case
    worst, n = 0.0, 0
    for name in case_names():
        c, host, q, prof, r = _golden_hp(name)
        osym, ometa = OC.genome_profile(host, c.m, c.k, c.mask_host)
        exp = OC.scan(q, OC.genome_ivom(osym, ometa, c.m, c.k), c.m, c.k, c.w, c.i, scaffolds_all=c.scaffolds_all)
        assert len(exp["kld"]) == len(r["cand"])
        ok = r["flag"] == H.OK
        worst, n = max(worst, _worst(exp["kld"], r, ok)), n + int(ok.sum())
    out["C oracle"] = (worst, n)
    return out


def _n_filtered(s):
    e = N.Encoded(s)
    return e.n - int(e.upper.sum()) >= 0.3 * e.n


def _pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def test_c_kld_is_calibrated_and_every_double_implementation_is_within_the_bound():
    cal = _calibration()
    for src, (worst, n) in cal.items():
        print("KLD calibration: %-13s worst normalised error %.2f over %d rows" % (src, worst, n))
    overall = max(w for w, _ in cal.values())
    print("C_KLD = %g (smallest power of two >= 4 x %.2f)" % (H.C_KLD, overall))
    assert all(n >= 200 for _, n in cal.values()), cal
    assert H.C_KLD == _pow2_at_least(4 * overall), (H.C_KLD, overall)
    assert all(w <= H.C_KLD for w, _ in cal.values())


def test_c_oracle_on_fuzz_cases_is_within_the_bound_and_its_sequential_sums():
    """The compiled C oracle on the first 50 cases of test_gpu_fuzz.py's generator (12 seeded rows each).  It normalises by
    Sw and Sg added up one max-mer after another, as the reference does, so its error also grows with the number m of
    max-mers: up to ~36 eps64 * scale on rows of 1 000-4 000 max-mers, where the same arithmetic with Sw, Sg summed exactly
    stays under ~3.  Hence this check adds H.sequential_sums_allowance to the bound and C_KLD is calibrated without these
    rows; the kernels sum Sw, Sg and T exactly, so the GPU tests hold them to the bound alone."""
    pick = np.random.default_rng(21)
    worst, n = 0.0, 0
    for block in range(2):
        rng = np.random.default_rng(1000 + block)           # test_gpu_fuzz.py's first blocks: the same cases
        for _ in range(25):
            c = random_case(rng)
            km, kx = c["kmin"], c["kmax"]
            prof = H.profile(c["seqs"], km, kx, c["mask_host"])
            osym, ometa = OC.genome_profile(c["seqs"], km, kx, c["mask_host"])
            assert np.array_equal(prof[0], osym) and tuple(prof[1]) == tuple(ometa)
            exp = OC.scan(c["seqs"], OC.genome_ivom(osym, ometa, km, kx), km, kx, c["w"], c["inc"], scaffolds_all=c["scaffolds_all"])
            allc = H.candidates(c["seqs"], c["w"], c["inc"], c["scaffolds_all"])
            sample = sorted(pick.permutation(len(allc))[:12].tolist()) if allc else []
            r = H.scan_hp(c["seqs"], prof, km, kx, c["w"], c["inc"], c["scaffolds_all"], cand=sample)
            if not len(r["cand"]):
                continue
            kept = [k for k, si, a, b, _, _ in allc if not _n_filtered(c["seqs"][si][a:b])]      # the C oracle's rows
            assert len(kept) == len(exp["kld"])
            at = {k: j for j, k in enumerate(kept)}
            j = np.array([at[int(k)] for k in r["cand"]])
            assert np.array_equal(exp["start"][j], r["start"]) and np.array_equal(exp["stop"][j], r["stop"])
            assert np.array_equal((exp["status"][j] & OC.ROW_ZERO_DIV) != 0, r["flag"] == H.ZERO_DIV)
            ok = r["flag"] == H.OK
            if not ok.any():
                continue
            kld = exp["kld"][j][ok]
            err = np.abs(kld - r["kld"][ok])
            assert (err <= H.bound(r["scale"][ok]) + H.sequential_sums_allowance(r["m"][ok], r["kld"][ok])).all()
            worst, n = max(worst, _worst(exp["kld"][j], r, ok)), n + int(ok.sum())
    print("C oracle on %d fuzz rows: worst normalised error %.2f (bound + sequential-sums allowance holds)" % (n, worst))
    assert n >= 200


def test_c_ivom_is_calibrated():
    """The normalised IVOM vectors of the double implementations (the golden window / genome vectors, which the reference's
    own IvomBuild wrote, and the numpy oracle's recursion on both sides) against the long-double pw, pg, per entry, in units
    of (K + 2) eps64 * value: C_IVOM is the smallest power of two at least four times the worst."""
    worst = {"golden": 0.0, "numpy oracle": 0.0}
    rows = 0
    for name in case_names():
        c, host, q, prof, r = _golden_hp(name)
        if c.k > 6:
            continue
        ig = N.genome_ivom_table(prof[0], prof[1], c.m, c.k)
        encs = [N.Encoded(s) for s in q]
        allc = H.candidates(q, c.w, c.i, c.scaffolds_all)
        for t, k in enumerate(r["cand"]):
            if r["flag"][t] != H.OK:
                continue
            present, pw, pg = r["ivom"][t]
            _, si, a, b, _, _ = allc[int(k)]
            win = encs[si].slice(a, b)
            cnt, _ = N.forward_counts(win, c.m, c.k)
            S = int(win.upper.sum())
            iw = N.genome_ivom_table(cnt, (win.n, 0, win.n - S), c.m, c.k)      # (the same recursion, D = (S - (x - 1)) * 2)
            dw, dg = np.zeros(4 ** c.k), np.zeros(4 ** c.k)
            dw[present] = iw[present] / iw[present].sum()
            dg[present] = ig[present] / ig[present].sum()
            worst["numpy oracle"] = max(worst["numpy oracle"], H.ivom_error(dw, present, pw, c.k), H.ivom_error(dg, present, pg, c.k))
            if c.window_ivom is not None:
                worst["golden"] = max(worst["golden"], H.ivom_error(c.window_ivom[t], present, pw, c.k),
                                      H.ivom_error(c.genome_ivom[t], present, pg, c.k))
            rows += 1
    for src, w in worst.items():
        print("IVOM calibration: %-13s worst normalised error %.2f" % (src, w))
    overall = max(worst.values())
    print("C_IVOM = %g (smallest power of two >= 4 x %.2f), %d rows" % (H.C_IVOM, overall, rows))
    assert rows >= 200
    assert H.C_IVOM == _pow2_at_least(4 * overall)


# ---- the test of the test: scan8_kernel.h's logarithm, emulated, and two subtly wrong variants of it -------------------------
LN2_D = 0.69314718055994530942


def log_tab_emulated(x, nbin=64, deg=6, bin_shift=0):
    """log_tab_n<nbin, deg> of scan8_kernel.h in numpy: x = m 2^k, m in [0.5, 1); bin i from m's top log2(nbin) mantissa
    bits; the table of frisk_abi.hip, u_i = 1/c_i rounded (c_i the bin's midpoint) and -ln u_i rounded; r = m u_i - 1 rounded
    once (the fma); log1p(r) by its Taylor polynomial of degree `deg` in Horner form; k ln2 + (-ln u_i) + log1p(r).
    bin_shift=1: the bin index one too high (kept inside the table)."""
    m, k = np.frexp(x)
    i = np.minimum(np.floor((m - 0.5) * 2 * nbin).astype(np.int64) + bin_shift, nbin - 1)
    u = 1.0 / (0.5 + (i + 0.5) / (2.0 * nbin))
    ly = (-np.log(u.astype(LD))).astype(np.float64)
    r = (m.astype(LD) * u.astype(LD) - 1).astype(np.float64)
    p = np.full_like(r, 1.0 / deg if deg & 1 else -1.0 / deg)
    for d in range(deg - 1, 1, -1):
        p = r * p + (1.0 / d if d & 1 else -1.0 / d)
    return (k * LN2_D + ly) + (r * r * p + r)


def _one_pass_kld(enc, ig, kmin, kmax, logf):
    """The kernels' scoring in double: Iw in closed form (sum c_x^2 4^x / D_x) / (sum c_x 4^x), the ratio Iw / Ig,
    T = sum Iw ln(Iw / Ig), KLD = (T / Sw - ln Sw + ln Sg) / ln 2."""
    present, cs, S = H.window_counts(enc, kmin, kmax)
    A, W = np.zeros(present.size), np.zeros(present.size)
    for t, c in enumerate(cs):
        x = kmin + t
        A += (c * c).astype(np.float64) * (4.0 ** x / ((S - (x - 1)) * 2))
        W += (c << (2 * x)).astype(np.float64)
    Iw, Ig = A / W, ig[present]
    T, Sw, Sg = np.sum(Iw * logf(Iw / Ig)), Iw.sum(), Ig.sum()
    return ((T / Sw - np.log(Sw)) + np.log(Sg)) / LN2_D


def test_the_bound_rejects_a_degraded_table_logarithm():
    """Golden rows of k8, k7, markov_m3k5, hq_k8 and k8_w2000 scored with the emulated log_tab_n: the shipped 64-bin, degree-6
    form is inside the bound on every row; a degree-4 polynomial (error ~1.8e-13, 57x under the flat 1e-11 of the parity tests)
    and the bin index one too high (~4e-14) each exceed it on at least one row."""
    variants = {"64 bins, degree 6": dict(), "64 bins, degree 4": dict(deg=4), "64 bins, degree 6, bin + 1": dict(bin_shift=1)}
    worst = dict.fromkeys(variants, 0.0)
    over = dict.fromkeys(variants, 0)
    for name in ("k8", "k7", "markov_m3k5", "hq_k8", "k8_w2000"):
        c, host, q, prof, r = _golden_hp(name)
        ig = N.genome_ivom_table(prof[0], prof[1], c.m, c.k)
        encs = [N.Encoded(s) for s in q]
        allc = H.candidates(q, c.w, c.i, c.scaffolds_all)
        for t, k in enumerate(r["cand"]):
            if r["flag"][t] != H.OK:
                continue
            _, si, a, b, _, _ = allc[int(k)]
            for v, kw in variants.items():
                kld = _one_pass_kld(encs[si].slice(a, b), ig, c.m, c.k, functools.partial(log_tab_emulated, **kw))
                e = float(H.normalised_error(kld, r["kld_hp"][t], r["scale"][t]))
                worst[v] = max(worst[v], e)
                over[v] += abs(kld - float(r["kld_hp"][t])) > H.bound(r["scale"][t])
    for v in variants:
        print("emulated log_tab_n, %-26s worst normalised error %8.2f, rows over the bound: %d" % (v, worst[v], over[v]))
    assert over["64 bins, degree 6"] == 0
    assert over["64 bins, degree 4"] >= 1
    assert over["64 bins, degree 6, bin + 1"] >= 1
