"""Per-k-mer oracle of the frisk_explain_ranges tests  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A range's KLD is the sum of the reference's summands (KLD, L465-470) over its present max-mers,
    t_k = pw_k ln(pw_k / pg_k) / ln 2,   pw = Iw / Sw,  pg = Ig / Sg.
explain_row() gives them per max-mer in x87 extended precision, from kld_oracle_hp.score_hp (which keeps the reference's
operation order), with the exact count of each max-mer and the per-k-mer scale
    s_k = pw_k (|ln(pw_k / pg_k)| + |ln Sw| + |ln Sg| + 1) / ln 2:
what an FP64 evaluation of t_k can lose - the rounding of its own logarithm, and the relative errors of the two normalisers, which
a one-pass form turns into the logarithms it subtracts.  Because sum pw = 1, the s_k of a row add up to the row's `scale` of
kld_oracle_hp, and the t_k to its KLD.

The per-term bound is  |term - t_k| <= C_TERM * eps64 * s_k.  C_TERM is calibrated as C_KLD and C_IVOM are, on the CPU and never
on a GPU (tests/test_explain_cpu.py): the smallest power of two that is at least four times the worst normalised error of two FP64
numpy restatements - the two-pass form pw (ln(pw / pg) / ln 2) and the one-pass form pw (ln(Iw / Ig) - ln Sw + ln Sg) / ln 2 - over
the scored rows of ranges_cases.range_set at every ranges_cases.ORDERS.  Measured there: worst 2.26 (orders 2..9, the two-pass
form), hence 16.
"""
import functools

import numpy as np

import kld_oracle_hp as H
import ranges_cases as R
from oracle import frisk_oracle_np as N

LD = H.LD
C_TERM = 16.0


def term_bound(s):
    return C_TERM * H.EPS64 * np.asarray(s, dtype=np.float64)


def explain_row(enc, prof, kmin, kmax):
    """One range (an N.Encoded slice) against a profile: score_hp's dict, plus - for a row of flag OK - count (the exact
    occurrences of each present max-mer), t_hp and s (long double, parallel to present, pw, pg)."""
    out = H.score_hp(enc, prof, kmin, kmax)
    if out["flag"] != H.OK:
        return out
    present, cw, _ = H.window_counts(enc, kmin, kmax)
    assert np.array_equal(present, out["present"])
    pw, pg = out["pw"], out["pg"]
    lr = np.log(pw / pg)
    out["count"] = cw[-1]
    out["t_hp"] = pw * lr / H.LN2
    out["s"] = pw * (np.abs(lr) + abs(np.log(out["sw"])) + abs(np.log(out["sg"])) + 1) / H.LN2
    return out


def explain_rows(seqs, prof, rows, kmin, kmax):
    """explain_row per (seq, start, stop) row; None for a row the N rule drops (L238)."""
    encs, out = {}, []
    for s, a, b in rows:
        if s not in encs:
            encs[s] = N.Encoded(seqs[s])
        enc = encs[s].slice(int(a), int(b))
        if enc.n - int(enc.upper.sum()) >= 0.3 * enc.n:
            out.append(None)
            continue
        out.append(explain_row(enc, prof, kmin, kmax))
    return out


@functools.lru_cache(maxsize=None)
def expected(kmin, kmax):
    """The range set of ranges_cases at (kmin, kmax) and its per-k-mer oracle rows, computed once and left unchanged."""
    rows = R.range_set(kmax)
    return rows, explain_rows(R.scaffolds(), R.profile(kmin, kmax), rows, kmin, kmax)


# ---- the two FP64 restatements C_TERM is calibrated on ----------------------------------------------------------------------------
def ivom_f64(cs, space, kmin):
    """kld_oracle_hp.ivom_ld in float64: the reference's recursion as a double implementation runs it."""
    W = np.zeros(cs[0].size, dtype=np.int64)
    I = np.zeros(cs[0].size, dtype=np.float64)
    for t, c in enumerate(cs):
        x = kmin + t
        wt = c << (2 * x)
        W = W + wt
        p = c.astype(np.float64) / float((space - (x - 1)) * 2)
        a = wt.astype(np.float64) / W.astype(np.float64)
        I = a * p if t == 0 else a * p + (1.0 - a) * I
    return I


def terms_f64(enc, prof, kmin, kmax):
    """(two-pass, one-pass) FP64 terms of a row of flag OK, parallel to the oracle's `present`."""
    sym, meta = prof
    present, cw, S = H.window_counts(enc, kmin, kmax)
    Iw = ivom_f64(cw, S, kmin)
    Ig = ivom_f64(H.genome_counts(sym, kmin, kmax, present), int(meta[0]) - int(meta[2]), kmin)
    Sw, Sg = Iw.sum(), Ig.sum()
    ln2 = float(np.log(2.0))
    pw, pg = Iw / Sw, Ig / Sg
    two = pw * (np.log(pw / pg) / ln2)
    one = pw * (np.log(Iw / Ig) - np.log(Sw) + np.log(Sg)) / ln2
    return two, one


def normalised_term_error(term, t_hp, s):
    """|term - t_hp| in units of eps64 * s (what C_TERM bounds), per k-mer."""
    d = np.abs(np.asarray(term, dtype=LD) - t_hp)
    return np.asarray(d / (LD(H.EPS64) * s), dtype=np.float64)


def calibration():
    """{(kmin, kmax): (worst of the two-pass form, worst of the one-pass form, scored rows)} over ranges_cases.ORDERS."""
    out = {}
    seqs = R.scaffolds()
    encs = {}
    for kmin, kmax in R.ORDERS:
        rows, exp = expected(kmin, kmax)
        prof = R.profile(kmin, kmax)
        w2 = w1 = 0.0
        n = 0
        for (s, a, b), e in zip(rows, exp):
            if e is None or e["flag"] != H.OK:
                continue
            if s not in encs:
                encs[s] = N.Encoded(seqs[s])
            two, one = terms_f64(encs[s].slice(int(a), int(b)), prof, kmin, kmax)
            w2 = max(w2, float(normalised_term_error(two, e["t_hp"], e["s"]).max()))
            w1 = max(w1, float(normalised_term_error(one, e["t_hp"], e["s"]).max()))
            n += 1
        out[(kmin, kmax)] = (w2, w1, n)
    return out
