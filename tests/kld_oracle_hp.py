"""Extended-precision restatement of the reference's KLD column  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reference scores a window as IvomBuild (frisk/__init__.py L426-446) on both sides followed by KLD (L465-470):
    I_x = a_x p_x + (1 - a_x) I_{x-1},   a_x = w_x / (w_kmin + .. + w_x),   w_x = c_x 4^x,   p_x = c_x / D_x
    pw = Iw / Sw,  pg = Ig / Sg,  KLD = sum pw ln(pw / pg) / ln 2
over the max-mers present in the window (Sw, Sg: the sums of the un-normalised IVOMs over those max-mers).  This module
evaluates exactly that in x87 extended precision (np.longdouble, 64-bit mantissa) from the exact integer counts of
oracle/frisk_oracle_np.py, so its result is ~2^11 times closer to the true value than any FP64 implementation can be.

Every FP64 implementation carries an error that scales with the conditioning of the row: the terms pw ln(pw/pg), and the
logarithms of Sw and Sg that a one-pass form (T/Sw - ln Sw + ln Sg) subtracts from each other.  Hence the per-row bound
    |KLD - KLD_hp| <= C_KLD * eps64 * scale,   scale = (sum pw |ln(pw/pg)| + |ln Sw| + |ln Sg| + 1) / ln 2
with one constant C_KLD, calibrated on the CPU against three double implementations (tests/test_kld_precision_cpu.py):
the smallest power of two that is at least four times the worst normalised error any of them shows.  It is not tuned
to what a GPU does.

The genome-side IVOM is evaluated only at the max-mers a window holds (gathered from the symmetric counts per order):
never over the dense 4^K table.
"""
import numpy as np

from oracle import frisk_oracle_np as N

assert np.finfo(np.longdouble).nmant >= 63, (
    "the KLD reference needs an extended-precision long double (x87, 64-bit mantissa); this platform's has %d bits: "
    "the precision tests would silently compare double against double" % (np.finfo(np.longdouble).nmant + 1))

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
LN2 = np.log(LD(2))

# per-row bound of the KLD column: C_KLD * eps64 * scale (calibrated in tests/test_kld_precision_cpu.py, not on a GPU)
C_KLD = 32.0
# per-entry bound of the normalised IVOM vectors: C_IVOM * (K + 2) * eps64 * value (calibrated the same way)
C_IVOM = 8.0

OK, ZERO_DIV, NO_MAXMER, DEGENERATE = 0, 2, 8, 16     # row flags (ZERO_DIV / NO_MAXMER: the library's status bits)


def bound(scale):
    return C_KLD * EPS64 * np.asarray(scale, dtype=np.float64)


def sequential_sums_allowance(m, kld):
    """What a double implementation that adds up the normalisers Sw and Sg one max-mer after another (the reference itself,
    the C oracle) may lose beyond bound(): each sum carries a relative error of up to (m - 1) eps64, which shifts every pw
    (pg) alike and reaches the KLD as (dSw (1 + KLD ln 2) + dSg) / ln 2.  The kernels sum Sw, Sg and T exactly (scan_kernel.h,
    ExactSum) and numpy pairwise: to them this allowance does not apply."""
    m = np.asarray(m, dtype=np.float64)
    return np.maximum(m - 1, 0) * EPS64 * (2 + np.abs(np.asarray(kld, dtype=np.float64)) * float(LN2)) / float(LN2)


def normalised_error(kld, kld_hp, scale):
    """|kld - kld_hp| in units of eps64 * scale (what C_KLD bounds)."""
    d = np.abs(np.asarray(kld, dtype=LD) - np.asarray(kld_hp, dtype=LD))
    return np.asarray(d / (LD(EPS64) * np.asarray(scale, dtype=LD)), dtype=np.float64)


def profile(seqs, kmin, kmax, mask_host=False):
    """(sym, meta): the genome side, from the numpy oracle's integer counts."""
    return N.genome_profile(seqs, kmin, kmax, mask_host)


def window_counts(enc, kmin, kmax):
    """(present, [c_kmin .. c_kmax], S): the distinct max-mers of an Encoded window (ascending codes), the forward counts of
    their x-prefixes per order (the words of N.forward_counts: every valid word of the window, one-base step), and the
    number of uppercase A/C/G/T (the S of D = (S - (x - 1)) * 2)."""
    codes, good = N._word_codes(enc.code, enc.valid, kmax)
    present, ctop = np.unique(codes[good], return_counts=True)
    cs = []
    for x in range(kmin, kmax):
        cx, gx = N._word_codes(enc.code, enc.valid, x)
        u, c = np.unique(cx[gx], return_counts=True)
        pre = present >> (2 * (kmax - x))
        j = np.searchsorted(u, pre)
        assert np.array_equal(u[j], pre) if present.size else True
        cs.append(c[j].astype(np.int64))
    cs.append(ctop.astype(np.int64))
    return present, cs, int(enc.upper.sum())


def genome_counts(sym, kmin, kmax, present):
    """[c_kmin .. c_kmax] of the genome at the given max-mers, gathered from the symmetric table per order."""
    return [np.asarray(sym[N.table_offset(kmin, x) + (present >> (2 * (kmax - x)))], dtype=np.int64) for x in range(kmin, kmax + 1)]


def ivom_ld(cs, space, kmin):
    """The reference's recursion in long double over parallel count vectors.  Returns (I, zero_div): zero_div where the
    reference divides by zero (a weight sum W_x = 0 or a divisor D_x = 0)."""
    W = np.zeros(cs[0].size, dtype=np.int64)
    I = np.zeros(cs[0].size, dtype=LD)
    for t, c in enumerate(cs):
        x = kmin + t
        wt = c << (2 * x)
        W = W + wt
        D = (space - (x - 1)) * 2
        if D == 0 or (W == 0).any():
            return None, True
        p = c.astype(LD) / LD(D)
        a = wt.astype(LD) / W.astype(LD)
        I = a * p if t == 0 else a * p + (LD(1) - a) * I
    return I, False


def score_hp(enc, prof, kmin, kmax):
    """One window (an N.Encoded slice) against a profile (sym, meta): dict(flag, kld, scale, m, sw, sg, present, pw, pg)."""
    sym, meta = prof
    present, cw, S = window_counts(enc, kmin, kmax)
    out = dict(flag=OK, kld=LD(0), scale=1.0 / float(LN2), m=int(present.size))
    if present.size == 0:
        out["flag"] = NO_MAXMER
        return out
    Iw, zw = ivom_ld(cw, S, kmin)
    Ig, zg = ivom_ld(genome_counts(sym, kmin, kmax, present), int(meta[0]) - int(meta[2]), kmin)
    if zw or zg:
        out["flag"] = ZERO_DIV
        return out
    Sw, Sg = Iw.sum(), Ig.sum()
    pw, pg = Iw / Sw, Ig / Sg
    if not ((pw > 0).all() and (pg > 0).all()):     # (negative divisors in a window of tiny, mostly soft-masked scaffolds)
        out["flag"] = DEGENERATE
        return out
    lr = np.log(pw / pg)
    out.update(kld=(pw * lr).sum() / LN2, sw=Sw, sg=Sg, present=present, pw=pw, pg=pg,
               scale=float(((pw * np.abs(lr)).sum() + abs(np.log(Sw)) + abs(np.log(Sg)) + 1) / LN2))
    return out


def candidates(seqs, w, inc, scaffolds_all=False):
    """Every candidate window in the library's numbering: (cand, seq, a, b, start, stop) per candidate, in order
    (N.iter_windows per scaffold, before the N filter)."""
    out, k = [], 0
    for si, s in enumerate(seqs):
        for a, b, start, stop in N.iter_windows(len(s), w, inc, scaffolds_all):
            out.append((k, si, a, b, start, stop))
            k += 1
    return out


def scan_hp(seqs, prof, kmin, kmax, w, inc, scaffolds_all=False, cand=None, keep_ivom=False):
    """Per KEPT row (the 30 % N filter of L213 / L238 applied), over the candidates named by `cand` (None: all; (c0, c1): a
    range; otherwise an iterable of candidate indices): dict of arrays cand, start, stop, flag, kld_hp (long double), kld
    (float64 of it), scale, m.  `seqs` are the scaffolds the windows come from; `prof` = profile(...) of the genome (in the
    query-file mode a different set of sequences).  keep_ivom=True adds per-row (present, pw, pg) under "ivom"."""
    encs = [N.Encoded(s) for s in seqs]
    allc = candidates(seqs, w, inc, scaffolds_all)
    if cand is None:
        sel = allc
    elif isinstance(cand, tuple):
        sel = allc[cand[0]:cand[1] if cand[1] >= 0 else len(allc)]
    else:
        sel = [allc[int(i)] for i in sorted(set(int(i) for i in cand))]
    rows = dict(cand=[], start=[], stop=[], flag=[], kld_hp=[], scale=[], m=[])
    ivoms = []
    for k, si, a, b, start, stop in sel:
        win = encs[si].slice(a, b)
        if win.n - int(win.upper.sum()) >= 0.3 * win.n:
            continue
        r = score_hp(win, prof, kmin, kmax)
        for f, v in (("cand", k), ("start", start), ("stop", stop), ("flag", r["flag"]), ("kld_hp", r["kld"]),
                     ("scale", r["scale"]), ("m", r["m"])):
            rows[f].append(v)
        if keep_ivom:
            ivoms.append((r.get("present"), r.get("pw"), r.get("pg")))
    out = {f: np.array(v, dtype=LD if f == "kld_hp" else (np.float64 if f == "scale" else np.int64)) for f, v in rows.items()}
    out["kld"] = out["kld_hp"].astype(np.float64)
    out["n_candidates"] = len(allc)
    if keep_ivom:
        out["ivom"] = ivoms
    return out


def ivom_error(got_dense, present, hp, K):
    """Worst per-entry error of a dense normalised IVOM vector (as frisk_scan_ivom writes it) against the long-double one, in
    units of (K + 2) eps64 * value; also checks that exactly the present max-mers carry weight."""
    nz = np.nonzero(got_dense)[0]
    assert np.array_equal(nz, present), "the set of present max-mers differs"
    g = np.asarray(got_dense[present], dtype=LD)
    return float(np.max(np.abs(g - hp) / ((K + 2) * LD(EPS64) * hp)))


def read_fasta(path):
    """The sequences of a FASTA file (the reference's reader), as strings."""
    from oracle import frisk_oracle as O
    return [s for _, s in O.iter_fasta(path)]
