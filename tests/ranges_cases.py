"""The scaffolds, the range set and the per-range oracle of the frisk_score_ranges tests  --  TEST INFRASTRUCTURE.

One range = one iteration of the reference's scan loop on the slice: oracle.frisk_oracle_np.score_window gives status, nn, GC and
the RIP indices (compared exactly), kld_oracle_hp.score_hp the KLD in extended precision and the row's scale (compared within
kld_oracle_hp.bound(scale), C_KLD = 32)."""
import functools

import numpy as np

import kld_oracle_hp as H
from oracle import frisk_oracle_np as N

KEPT, ZERO_WEIGHT, JUMPBACK, NO_MAXMER = 1, 2, 4, 8
T_SHORT = 512                   # FRISK_RANGE_NT: the short form's thread count
ORDERS = [(1, 8), (1, 6), (3, 5), (8, 8), (1, 7), (2, 9)]
ACGT = np.frombuffer(b"ATGC", dtype=np.uint8)


def _bases(rng, n, gc):
    return rng.choice(ACGT, size=n, p=[(1 - gc) / 2, (1 - gc) / 2, gc / 2, gc / 2]).tobytes()


@functools.lru_cache(maxsize=None)
def scaffolds():
    rng = np.random.default_rng(20240611)
    s0 = _bases(rng, 1500, 0.5) + b"N" * 40 + _bases(rng, 1000, 0.5) + _bases(rng, 300, 0.5).lower() + _bases(rng, 1200, 0.5)
    s1 = bytearray(_bases(rng, 70000, 0.3))
    s1[30000:42000] = _bases(rng, 12000, 0.7)
    s2 = b"".join(_bases(rng, 9, 0.5) + b"N" for _ in range(7000))
    s3 = b"ACGTTGCAacg"
    return [s0, bytes(s1), s2, s3]


def range_set(kmax):
    """(seq, start, stop) rows, 0-based half-open."""
    seqs = scaffolds()
    n0, n1, n2 = len(seqs[0]), len(seqs[1]), len(seqs[2])
    rows = []
    for r in (0, 1, 15, 16, 17, 31):
        for ln in (kmax - 1, kmax, kmax + 1, 31, 32, 33, 63, 64, 65, T_SHORT - 1, T_SHORT, T_SHORT + 1):
            rows.append((0, 64 + r, 64 + r + ln))
    rows += [(0, n0 - 100, n0), (0, 0, 77),
             (0, 1400, 1500), (0, 1540, 1640), (0, 1450, 1590), (0, 1505, 1535),       # beside, across and inside the N run
             (0, 2400, 3000), (0, 2540, 2840), (0, 1495, 1545), (0, 0, n0)]
    rows += [(1, 0, 65535), (1, 0, 65536), (1, 3, 70000), (1, 29000, 43000), (1, 0, n1)]
    rows += [(2, 0, 65535), (2, 5, 65541), (2, 0, n2)]
    rows += [(3, 0, 8), (3, 0, 11), (3, 1, 9)]
    return rows


def arrays(rows):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.int32), a[:, 1].copy(), a[:, 2].copy()


@functools.lru_cache(maxsize=None)
def profile(kmin, kmax):
    return H.profile(scaffolds(), kmin, kmax)


@functools.lru_cache(maxsize=None)
def _ig(kmin, kmax):
    sym, meta = profile(kmin, kmax)
    return N.genome_ivom_table(sym, meta, kmin, kmax)


def expect_rows(seqs, prof, ig, rows, kmin, kmax):
    """Per row: dict(status, nn, gc, rip (None without), flag, kld_hp, scale) - the reference's iteration on the slice."""
    encs = {}
    rip = kmin <= 2 <= kmax
    out = []
    nan = float("nan")
    for s, a, b in rows:
        if s not in encs:
            encs[s] = seqs[s] if isinstance(seqs[s], N.Encoded) else N.Encoded(seqs[s])
        enc = encs[s].slice(int(a), int(b))
        n, S = enc.n, int(enc.upper.sum())
        e = dict(nn=n - S, status=0, gc=nan, rip=[nan, nan, nan] if rip else None, flag=None, kld_hp=None, scale=None)
        if n - S >= 0.3 * n:                                    # L238: left unscored
            out.append(e)
            continue
        row = N.score_window(enc, ig, kmin, kmax, rip)
        hp = H.score_hp(enc, prof, kmin, kmax)
        assert ("error" in row) == (hp["flag"] == H.ZERO_DIV), (s, a, b)
        e["status"] = KEPT | (ZERO_WEIGHT if hp["flag"] == H.ZERO_DIV else 0) | (NO_MAXMER if hp["flag"] == H.NO_MAXMER else 0)
        e["gc"] = row["GC"]
        if rip:
            e["rip"] = row["RIP"]
        e.update(flag=hp["flag"], kld_hp=hp["kld"], scale=hp["scale"])
        out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def expected(kmin, kmax):
    """The range set of (kmin, kmax) and its oracle rows, computed once."""
    rows = range_set(kmax)
    return rows, expect_rows(scaffolds(), profile(kmin, kmax), _ig(kmin, kmax), rows, kmin, kmax)


OWN = object()          # engine(): this module's scaffolds / their profile


def engine(kmin, kmax, seqs=OWN, prof=OWN):
    """An Engine with `seqs` resident (default: scaffolds(); None: no batch) and the profile `prof` = (sym, meta) installed (default:
    profile(kmin, kmax); None: no profile)."""
    from frisk_amd.engine import Engine
    e = Engine(kmin, kmax)
    if seqs is not None:
        e.load(scaffolds() if seqs is OWN else seqs)
    if prof is not None:
        sym, meta = profile(kmin, kmax) if prof is OWN else prof
        e.profile_set(sym, *[int(v) for v in meta])
    return e


def score_columns(rip):
    return ["status", "nn", "kld", "gc"] + (["pi", "si", "cri"] if rip else [])


def same_columns(a, b, cols, ia=None, ib=None, what=""):
    """Asserts that the columns `cols` of two results hold the same bytes (rows ia of a against rows ib of b); returns True."""
    for c in cols:
        x, y = getattr(a, c), getattr(b, c)
        x = x if ia is None else x[ia]
        y = y if ib is None else y[ib]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, c)
    return True


def classes(exp):
    """(dropped by the N rule, without a max-mer, ZeroDivisionError, degenerate) counts of oracle rows."""
    return (sum(e["status"] == 0 for e in exp), sum(e["flag"] == H.NO_MAXMER for e in exp),
            sum(e["flag"] == H.ZERO_DIV for e in exp), sum(e["flag"] == H.DEGENERATE for e in exp))


def check(tag, res, exp, rip=None):
    """Every row of a score_ranges result against its oracle row: status, nn, GC and RIP exactly, KLD within the row's bound.
    Returns (and prints) the worst normalised KLD error."""
    from golden_util import same_float
    assert len(res) == len(exp), tag
    worst = 0.0
    for r, e in enumerate(exp):
        where = "%s row %d" % (tag, r)
        assert int(res.status[r]) == e["status"], (where, int(res.status[r]), e["status"])
        assert int(res.nn[r]) == e["nn"], where
        assert same_float(float(res.gc[r]), e["gc"]), (where, float(res.gc[r]), e["gc"])
        if e["rip"] is not None and res.pi is not None:
            got = [float(res.pi[r]), float(res.si[r]), float(res.cri[r])]
            assert all(same_float(g, w) for g, w in zip(got, e["rip"])), (where, got, e["rip"])
        k = float(res.kld[r])
        if e["status"] == 0 or e["flag"] == H.ZERO_DIV:
            assert k != k, (where, k)
        elif e["flag"] == H.NO_MAXMER:
            assert k == 0.0, (where, k)
        else:
            assert e["flag"] == H.OK, where
            err = abs(np.longdouble(k) - e["kld_hp"])
            worst = max(worst, float(H.normalised_error(k, e["kld_hp"], e["scale"])))
            assert err <= H.bound(e["scale"]), "%s: |dKLD| %.3g over the bound %.3g (normalised %.2f, C_KLD = %g)" % (
                where, float(err), float(H.bound(e["scale"])), float(H.normalised_error(k, e["kld_hp"], e["scale"])), H.C_KLD)
    print("%-44s rows %4d  worst normalised KLD error %6.2f" % (tag, len(exp), worst))
    return worst
