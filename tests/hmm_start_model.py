"""Float64 models of the HMM's deterministic start in both layouts, and of the first EM rounds in the device's layout  --  TEST
INFRASTRUCTURE, NOT PRODUCT CODE.

The start (GaussianHMM2._init) restated sum for sum in the order of
  * layout "device": hmm_init_range / hmm_init_range_final / hmm_init_assign / hmm_init_var / hmm_reduce_rows of
    frisk_amd/csrc/hmm_kernels.h - C = clamp(n / 256, 1, 1024) chunks [n c / C, n (c + 1) / C), thread tid of 256 adds the windows
    a + tid, a + tid + 256, .. in order, a tree over the 256 threads, then the chunks c = tid, tid + 256, .. and the tree again;
  * layout "host": frisk_hmm::init of csrc/hmm_host.h - minimum, maximum, sum and variance serially over the sequence, a 2-means
    assignment over clamp(n / 4096, 1, 256) pieces (each serially, then the pieces in order).
The start has no transcendental function and the library is built without fused operations, so a model is its layout's result bit
for bit (asserted for the host one in tests/test_hmm_start_cpu.py).  numpy does the adding, in exactly that order: a padded zero
(x + 0.0 == x) stands for a window a thread does not have, and numpy.cumsum adds from left to right.
`fit` continues with `rounds` EM rounds: tests/hmm_piece_model.py's E step, hmm.py's M step, the covariance sums in the order of
hmm_covar_walk + hmm_reduce_rows.
Two uses, as for hmm_piece_model: the distance from tests/hmm_oracle_hp.py is the error of correct double arithmetic in that
layout, and `defect=` seeds one of DEFECTS, which the comparison the GPU test uses must reject.
"""
import numpy as np

import hmm_piece_model as PM

PARTS = 1024              # frisk_hmm_gpu::PARTS
RED_T = 256               # frisk_hmm_gpu::RED_T
HOST_PIECES = 256         # frisk_hmm::PIECES
HOST_MIN = 4096           # windows per piece of frisk_hmm::init's assignment, at least
HOST_MIN_E = 2048         # .. of frisk_hmm::e_step

DEFECTS = (
    "chunk_last_window_dropped",      # every chunk's (piece's, serial loop's) last window left out
    "last_chunk_not_in_range",        # the minimum and maximum taken over the chunks but the last (device layout, C >= 2)
    "ties_to_centre_1",               # `<` for `<=` in the assignment
    "new_centres_kept",               # the NEW centres kept when the stop rule is met
    "variance_about_centre_0",        # the variance taken about the lower centre instead of the mean
    "chunk_count_one_short_at_cap",   # at C == PARTS the kernels run and are summed over PARTS - 1 chunks of the PARTS bounds
    "one_pass_variance",              # sum x^2 / n - mean^2
)
FIT_DEFECTS = (
    "covars_about_old_means",         # the M step's covariance sums about the means the E step used
    "covars_prior_left_out",          # covars_prior not added
)


def parts_of(n):
    return min(PARTS, max(1, n // RED_T))


def host_parts_of(n):
    return min(HOST_PIECES, max(1, n // HOST_MIN))


def host_pieces_of(n):
    return min(HOST_PIECES, max(1, n // HOST_MIN_E))


def bounds(n, C):
    return (n * np.arange(C + 1, dtype=np.int64)) // C


def _tree(s):
    """The 256-wide tree: sh[tid] += sh[tid + h] for h = 128, 64, .., 1 (last axis)."""
    s = np.array(s, dtype=np.float64)
    h = RED_T // 2
    while h > 0:
        s[..., :h] = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def _strided(rows):
    """Thread tid adds rows tid, tid + 256, .. in order, then the tree (hmm_reduce_rows, hmm_init_range_final)."""
    rows = np.asarray(rows, dtype=np.float64)
    K = max(1, -(-rows.size // RED_T))
    m = np.zeros(K * RED_T)
    m[:rows.size] = rows
    m = m.reshape(K, RED_T)
    s = m[0].copy()
    for k in range(1, K):
        s = s + m[k]
    return float(_tree(s))


class Device:
    def __init__(self, n, defect=None):
        C = parts_of(n)
        cut = bounds(n, C)
        a, b = cut[:-1], cut[1:]
        if defect == "chunk_last_window_dropped":
            b = b - 1
        if defect == "chunk_count_one_short_at_cap" and C == PARTS:
            a, b = a[:-1], b[:-1]
        self.range_rows = a.size - 1 if (defect == "last_chunk_not_in_range" and a.size >= 2) else a.size
        K = max(1, -(-int((b - a).max()) // RED_T))
        idx = a[:, None, None] + (np.arange(K, dtype=np.int64) * RED_T)[None, :, None] + np.arange(RED_T, dtype=np.int64)[None, None, :]
        self.valid = idx < b[:, None, None]
        self.idx = np.where(self.valid, idx, 0)

    def chunks(self, v):
        """Every chunk's sum: a thread's windows in order, then the tree."""
        m = np.where(self.valid, v[self.idx], 0.0)
        s = m[:, 0]
        for k in range(1, m.shape[1]):
            s = s + m[:, k]
        return _tree(s)

    def total(self, v):
        return _strided(self.chunks(v))

    assign = total

    def lo_hi(self, x):
        r = self.range_rows
        v = x[self.idx]
        return (float(np.where(self.valid, v, np.inf)[:r].min(initial=np.inf)), float(np.where(self.valid, v, -np.inf)[:r].max(initial=-np.inf)))


class Host:
    def __init__(self, n, defect=None):
        self.cut = bounds(n, host_parts_of(n))
        self.drop = 1 if defect == "chunk_last_window_dropped" else 0

    @staticmethod
    def _serial(v):
        return float(np.cumsum(v)[-1]) if v.size else 0.0

    def total(self, v):
        return self._serial(v[:v.size - self.drop])

    def assign(self, v):
        return self._serial(np.array([self._serial(v[a:b - self.drop]) for a, b in zip(self.cut[:-1], self.cut[1:])]))

    def lo_hi(self, x):
        v = x[:x.size - self.drop]
        return (float(v.min(initial=np.inf)), float(v.max(initial=-np.inf)))


def start(x, layout="device", defect=None, min_covar=1e-3):
    """(means [2], covar, rounds) in float64, in the order of `layout`."""
    assert layout in ("device", "host") and (defect is None or defect in DEFECTS)
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    L = (Device if layout == "device" else Host)(n, defect)
    with np.errstate(all="ignore"):
        lo, hi = L.lo_hi(x)
        mu = L.total(x) / float(n)
        c = [lo, hi]
        rounds = 0
        for _ in range(100):
            rounds += 1
            d0, d1 = np.abs(x - c[0]), np.abs(x - c[1])
            lab0 = (d0 < d1) if defect == "ties_to_centre_1" else (d0 <= d1)
            s0, n0 = L.assign(np.where(lab0, x, 0.0)), L.assign(lab0.astype(np.float64))
            s1, n1 = L.assign(np.where(lab0, 0.0, x)), L.assign((~lab0).astype(np.float64))
            nw = [s0 / n0 if n0 > 0 else c[0], s1 / n1 if n1 > 0 else c[1]]
            if abs(nw[0] - c[0]) <= 1e-8 + 1e-5 * abs(c[0]) and abs(nw[1] - c[1]) <= 1e-8 + 1e-5 * abs(c[1]):
                if defect == "new_centres_kept":
                    c = nw
                break
            c = nw
        means = [min(c[0], c[1]), max(c[0], c[1])]
        if defect == "variance_about_centre_0":
            mu = means[0]
        if defect == "one_pass_variance":
            covar = L.total(x * x) / float(n) - mu * mu + min_covar
        else:
            d = x - mu
            covar = L.total(d * d) / float(n) + min_covar
    return means, float(covar), rounds


def _cov_sums(sq, cut, reduce_rows):
    out = []
    for j in (0, 1):
        col = sq[:, j]
        out.append(reduce_rows([float(np.cumsum(col[a:b])[-1]) if b > a else 0.0 for a, b in zip(cut[:-1], cut[1:])]))
    return np.array(out)


def fit(x, rounds, defect=None, min_covar=1e-3, covars_prior=1e-2):
    """`rounds` EM rounds from the start, in the device's layout (GaussianHMM2(native="gpu", n_iter=rounds, tol=-1e300).fit): a list
    of (parameters as H.params gives them, log-likelihood of the round's E step) for every round."""
    assert defect is None or defect in DEFECTS + FIT_DEFECTS
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    means, covar, _r = start(x, "device", defect if defect in DEFECTS else None, min_covar)
    model = dict(means=means, covars=[covar, covar], start=[0.5, 0.5], trans=[[0.5, 0.5], [0.5, 0.5]])
    cut = PM.bounds(n, PM.pieces_of(n))
    out = []
    for _ in range(rounds):
        post, S, ll = PM.e_step(x, model)
        sp = post[0] / (post[0, 0] + post[0, 1])
        trans = np.full((2, 2), 0.5)
        if n > 1:
            for i in (0, 1):
                row = S[4 + 2 * i] + S[5 + 2 * i]
                if row > 0:
                    trans[i] = [S[4 + 2 * i] / row, S[5 + 2 * i] / row]
        mu = np.array([S[2] / S[0], S[3] / S[1]])
        about = np.array(model["means"]) if defect == "covars_about_old_means" else mu
        d = x[:, None] - about[None, :]
        cc = _cov_sums(post * (d * d), cut, PM._reduce_rows)
        prior = 0.0 if defect == "covars_prior_left_out" else covars_prior
        cv = np.maximum((prior + cc) / S[0:2], 1e-300)
        model = dict(means=mu.tolist(), covars=cv.tolist(), start=sp.tolist(), trans=trans.tolist())
        out.append(({"means_": mu.tolist(), "covars_": cv.tolist(), "startprob_": sp.tolist(), "transmat_": trans.ravel().tolist()}, float(ll)))
    return out
