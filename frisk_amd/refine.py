"""Base-resolution region boundaries by a likelihood-ratio change point - host specification of frisk_refine_ranges.

`refine_rows()` restates csrc/refine_kernels.h in numpy and produces the same integers, as nullmodel.py does for the null
generator.  The definition (include/frisk_hip.h states it too; DESIGN.md section 17 says why it is this one):

  * row     : (seq, a, b), 0-based half-open on a batch of scaffolds; F = flank (1 .. MAX_FLANK), r = order (kmin <= r + 1 <= kmax).
              Fe = min(F, (b - a) // 4); the core is [a + Fe, b - Fe), counted as frisk_score_ranges counts a slice: no word reaches
              past its ends, lowercase counts in words.  status and nn are the core's: nn = its positions that are not uppercase
              A/C/G/T, status = ROW_KEPT, | ROW_NO_MAXMER without a valid kmax-mer, | ROW_ZERO_WEIGHT with one and kmin - 1 <= S <=
              kmax - 1 (S = length - nn); the genome's weights are not looked at.  Fe = 0 (fewer than 4 bases) or a core the N rule
              drops (nn >= 0.3 * length, status 0): new_start = a, new_stop = b, both gains 0, flank_used = Fe.
  * models  : digits A, T, G, C = 0..3, first base most significant; the word c of r + 1 letters has the context c >> 2.
              island n_i(c) = the core's count of c, host n_h(c) = sym_{r+1}[c] of the finalised profile; T(ctx) = the four-sum.
              lp(n, T) = flog2(n + 1) - flog2(T + 4) (Laplace), qtab(c) = lp(n_i, T_i) - lp(n_h, T_h): int64, units of 2^-32 bit
  * flog2   : x = m * 2^e with m a Q1.63 mantissa; 32 squarings of m (128-bit products, truncated to 64 bits) give the fraction's
              bits.  0 <= 2^32 log2 x - flog2(x) < 1 + 2^-20.  Integers only: every sum below is exact, whatever its order
  * per base: q_j = qtab(word of bases [j - r, j], upper-cased) when j - r >= 0 and its r + 1 bases are all A/C/G/T, else 0
  * cuts    : start: G_s(t) = sum_{j = t}^{a + Fe - 1} q_j over t in [max(0, a - Fe), a + Fe]; new_start = the LARGEST t of maximal G_s
              stop : G_e(u) = sum_{j = b - Fe}^{u - 1} q_j over u in [b - Fe, min(L, b + Fe)]; new_stop = the SMALLEST u of maximal G_e
              gain_start = G_s(new_start) - G_s(a), gain_stop = G_e(new_stop) - G_e(b), both >= 0.  On a tie the shorter region wins.
"""
import numpy as np

from .engine import table_offset
from .nullmodel import mulhi64

MAX_FLANK = 65536
ROW_KEPT, ROW_ZERO_WEIGHT, ROW_NO_MAXMER = 1, 2, 8
_LUT = np.full(256, -1, dtype=np.int64)
for _i, _pair in enumerate(("Aa", "Tt", "Gg", "Cc")):
    for _ch in _pair:
        _LUT[ord(_ch)] = _i
_UPPER = np.zeros(256, dtype=bool)
_UPPER[[ord(ch) for ch in "ACGT"]] = True


def flog2(x):
    """int64 array: floor-ish 2^32 * log2(x) of integers 1 <= x < 2^63, by the definition above (exactly the device's bits)."""
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64)
    if x.size and (int(x.min()) < 1 or int(x.max()) >= 1 << 63):
        raise ValueError("flog2 takes 1 <= x < 2^63")
    e = np.zeros(x.shape, dtype=np.uint64)
    t = x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        up = (t >> np.uint64(s)) != 0
        e = np.where(up, e + np.uint64(s), e)
        t = np.where(up, t >> np.uint64(s), t)
    m = x << (np.uint64(63) - e)
    f = np.zeros(x.shape, dtype=np.uint64)
    top = np.uint64(1 << 63)
    with np.errstate(over="ignore"):
        for _ in range(32):
            hi, lo = mulhi64(m, m), m * m
            big = hi >= top
            f = (f << np.uint64(1)) | big.astype(np.uint64)
            m = np.where(big, hi, (hi << np.uint64(1)) | (lo >> np.uint64(63)))
    return ((e << np.uint64(32)) + f).astype(np.int64)


def lp_table(counts):
    """lp(n(c), T(c >> 2)) of a table of 4^x counts, int64."""
    n = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    total = n.sum(axis=1, keepdims=True)
    return (flog2(n.reshape(-1) + 1).reshape(-1, 4) - flog2(total.reshape(-1) + 4).reshape(-1, 1)).reshape(-1)


def qtab(island, host):
    """qtab(c) of the island's and the host's counts of the 4^(r+1) words, int64 in units of 2^-32 bit."""
    return lp_table(island) - lp_table(host)


class _Scaffold:
    """A scaffold's digits (-1: not A/C/G/T of either case), uppercase flags and, per order, the word that ends at each base."""

    def __init__(self, seq):
        raw = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
        self.n = raw.size
        self.digit = _LUT[raw]
        self.upper = _UPPER[raw]
        self._words = {}

    def words(self, x):
        """int64 (n,): the code of the x-mer of bases [j - x + 1, j], -1 where it is not valid."""
        if x not in self._words:
            w = np.full(self.n, -1, dtype=np.int64)
            if self.n >= x:
                m = self.n - x + 1
                code = np.zeros(m, dtype=np.int64)
                bad = np.zeros(m, dtype=bool)
                for p in range(x):
                    d = self.digit[p:p + m]
                    code = (code << 2) | np.maximum(d, 0)
                    bad |= d < 0
                w[x - 1:] = np.where(bad, -1, code)
            self._words[x] = w
        return self._words[x]


class RefineResult:
    """Columns of refine_rows / Engine.refine_ranges, one entry per row."""
    COLUMNS = ["status", "nn", "new_start", "new_stop", "gain_start", "gain_stop", "flank_used"]

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return int(self.status.size)


def check_args(kmin, kmax, flank, order):
    """ValueError for a flank or an order that frisk_refine_ranges refuses."""
    if not 1 <= int(flank) <= MAX_FLANK:
        raise ValueError("flank outside 1 .. %d" % MAX_FLANK)
    if int(order) < 0 or not kmin <= int(order) + 1 <= kmax:
        raise ValueError("the chain of order r reads the counts of order r + 1, which must lie in kmin .. kmax")


def _host_lp(sym, kmin, kmax, flank, order):
    sym = np.asarray(sym, dtype=np.int64)
    if kmax is None:
        kmax = kmin
        while table_offset(kmin, kmax + 1) < sym.size:
            kmax += 1
    check_args(kmin, kmax, flank, order)
    off = table_offset(kmin, int(order) + 1)
    return kmax, lp_table(sym[off:off + 4 ** (int(order) + 1)])


def _cuts(sc, host_lp, a, b, Fe, r):
    """(t, G_s(t)), (u, G_e(u)) of a row whose core is kept, Fe > 0: both searches' candidates and their sums, int64."""
    x = r + 1
    ca, cb = a + Fe, b - Fe
    w = sc.words(x)
    core = w[ca + r:cb]                                             # the words that lie in the core
    island = np.bincount(core[core >= 0], minlength=4 ** x).astype(np.int64)
    total = island.reshape(-1, 4).sum(axis=1)

    def q(lo, hi):                                                  # q_j of lo <= j < hi; only the words that occur are evaluated
        wj = w[lo:hi]
        out = np.zeros(wj.size, dtype=np.int64)
        u, inv = np.unique(wj[wj >= 0], return_inverse=True)
        if u.size:
            out[wj >= 0] = ((flog2(island[u] + 1) - flog2(total[u >> 2] + 4)) - host_lp[u])[inv]
        return out
    lo_s, hi_s = max(0, a - Fe), a + Fe
    Gs = np.concatenate([np.cumsum(q(lo_s, hi_s)[::-1])[::-1], [0]])       # G_s(t), t = lo_s .. hi_s
    lo_e, hi_e = b - Fe, min(sc.n, b + Fe)
    Ge = np.concatenate([[0], np.cumsum(q(lo_e, hi_e))])                    # G_e(u), u = lo_e .. hi_e
    return (np.arange(lo_s, hi_s + 1), Gs), (np.arange(lo_e, hi_e + 1), Ge)


def cut_profiles(seqs, sym, kmin, row, flank, order, kmax=None):
    """((t, G_s), (u, G_e)) of one row: every candidate cut of both searches with its cumulative log-likelihood ratio (int64, units of
    2^-32 bit) - what refine_rows takes its arg-maxima from.  None for a row that is not refined (Fe = 0, or the N rule drops its core)."""
    res = refine_rows(seqs, sym, kmin, [row], flank, order, kmax=kmax)
    Fe = int(res.flank_used[0])
    if Fe == 0 or not int(res.status[0]) & ROW_KEPT:
        return None
    kmax, host_lp = _host_lp(sym, kmin, kmax, flank, order)
    s, a, b = (int(v) for v in row)
    return _cuts(_Scaffold(seqs[s]), host_lp, a, b, Fe, int(order))


def refine_rows(seqs, sym, kmin, rows, flank, order, kmax=None):
    """The columns frisk_refine_ranges writes for `rows` = (seq, a, b) on the batch `seqs` (bytes or str each) under the finalised
    profile's symmetric counts `sym` (orders from kmin, as Engine.profile_get returns them).  kmax: the engine's (default: the
    highest order `sym` holds)."""
    kmax, host_lp = _host_lp(sym, kmin, kmax, flank, order)
    F, r = int(flank), int(order)
    scaf = {}
    n = len(rows)
    res = RefineResult(status=np.zeros(n, np.uint32), nn=np.zeros(n, np.int64), new_start=np.zeros(n, np.int64),
                       new_stop=np.zeros(n, np.int64), gain_start=np.zeros(n, np.int64), gain_stop=np.zeros(n, np.int64),
                       flank_used=np.zeros(n, np.int64))
    for i, (s, a, b) in enumerate(rows):
        s, a, b = int(s), int(a), int(b)
        if s not in scaf:
            scaf[s] = _Scaffold(seqs[s])
        sc = scaf[s]
        if not (0 <= a < b <= sc.n):
            raise ValueError("row %d: range outside the scaffold (or empty)" % i)
        Fe = min(F, (b - a) // 4)
        ca, cb = a + Fe, b - Fe
        S = int(sc.upper[ca:cb].sum())
        nn = (cb - ca) - S
        res.nn[i], res.new_start[i], res.new_stop[i], res.flank_used[i] = nn, a, b, Fe
        if float(nn) >= 0.3 * float(cb - ca):
            continue
        ntop = int((sc.words(kmax)[ca + kmax - 1:cb] >= 0).sum())
        res.status[i] = ROW_KEPT | (ROW_NO_MAXMER if ntop == 0 else 0) | (ROW_ZERO_WEIGHT if ntop > 0 and kmin - 1 <= S <= kmax - 1 else 0)
        if Fe == 0:
            continue
        (t, Gs), (u, Ge) = _cuts(sc, host_lp, a, b, Fe, r)
        k = Gs.size - 1 - int(np.argmax(Gs[::-1]))                  # the LARGEST t of maximal G_s
        res.new_start[i], res.gain_start[i] = t[k], Gs[k] - Gs[a - t[0]]
        k = int(np.argmax(Ge))                                      # the SMALLEST u of maximal G_e
        res.new_stop[i], res.gain_stop[i] = u[k], Ge[k] - Ge[b - u[0]]
    return res


def default_order(kmin, kmax):
    """The order python -m frisk_amd.regions --refine uses without --refineOrder: low, because a core of a few kilobases cannot
    train a long context."""
    return min(max(2, kmin - 1), kmax - 1)
