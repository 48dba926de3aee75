"""Float64 model of the device E step's piece scheme  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A Python restatement, pass for pass, of the five E-step kernels of frisk_amd/csrc/hmm_kernels.h (hmm_emit_product, hmm_cuts'
two serial passes, hmm_forward_walk with its four-to-a-logarithm flush, hmm_backward_walk reading the cut vector at a piece's first
window, and the fixed-order sums), with the piece function as an argument.  Nothing on the CPU has the device's layout otherwise
(csrc/hmm_host.h cuts at n / 2048, the device at n / 32).  Two uses, both without a GPU:
  * tolerance: its distance from tests/hmm_oracle_hp.py is the error of CORRECT double arithmetic in the device's layout;
  * sensitivity: `defect=` seeds one of DEFECTS, and the comparison the GPU test uses must reject every one of them.
Python floats are IEEE doubles and no operation is fused, as in the library (built with -ffp-contract=off); math.exp / math.log
are the host's, the device's differ by an ulp or so - which is part of what the tolerance's factor is for.
"""
import math

import numpy as np

PIECES = 16384            # frisk_hmm_gpu::PIECES
MIN_STEPS = 32            # frisk_hmm_gpu::MIN_STEPS
RED_T = 256
LOG2PI = 1.8378770664093454835606594728112

DEFECTS = (
    "cut_from_neighbour",       # the forward cut vector taken from the neighbouring piece
    "beta_edge_of_next",        # the beta edge of piece p + 1 used for piece p
    "first_step_not_skipped",   # the first window's step multiplied into piece 0's product
    "xi_from_posterior",        # a piece's first transition posterior from the previous window's POSTERIOR (the overwrite)
    "first_scale_left_out",     # the log-scale of a piece's first step left out
    "flush_drops_held",         # the held product dropped at a piece's end
)


def pieces_of(n):
    return min(PIECES, max(1, n // MIN_STEPS))


def bounds(n, P):
    """[a_0, a_1, .., a_P]: piece p is [a_p, a_(p+1))."""
    return [n * p // P for p in range(P + 1)]


def _reduce_rows(rows):
    """hmm_reduce_rows: thread t adds rows t, t + 256, .. in order, then a tree over the 256 threads."""
    sh = [0.0] * RED_T
    for t in range(min(RED_T, len(rows))):
        s = 0.0
        for r in range(t, len(rows), RED_T):
            s += rows[r]
        sh[t] = s
    h = RED_T // 2
    while h > 0:
        for t in range(h):
            sh[t] += sh[t + h]
        h //= 2
    return sh[0]


def e_step(x, model, pieces=pieces_of, defect=None):
    """(posteriors n x 2 float64, stats[8] float64, loglik float)"""
    assert defect is None or defect in DEFECTS
    x = [float(v) for v in np.asarray(x, dtype=np.float64)]
    n = len(x)
    mu0, mu1 = (float(v) for v in model["means"])
    lc0, lc1 = (math.log(float(v)) for v in model["covars"])
    ic0, ic1 = (1.0 / float(v) for v in model["covars"])
    pi0, pi1 = (float(v) for v in model["start"])
    (a00, a01), (a10, a11) = ((float(v) for v in row) for row in model["trans"])
    P = pieces(n)
    cut = bounds(n, P)
    B0, B1 = [0.0] * n, [0.0] * n
    pm = [None] * P
    acc = [[0.0] * 10 for _ in range(P)]
    # 1. hmm_emit_product
    for p in range(P):
        m00, m01, m10, m11, ll = 1.0, 0.0, 0.0, 1.0, 0.0
        for t in range(cut[p], cut[p + 1]):
            d0, d1 = x[t] - mu0, x[t] - mu1
            l0, l1 = -0.5 * ((LOG2PI + lc0) + d0 * d0 * ic0), -0.5 * ((LOG2PI + lc1) + d1 * d1 * ic1)
            mx = max(l0, l1)
            b0, b1 = math.exp(l0 - mx), math.exp(l1 - mx)
            B0[t], B1[t] = b0, b1
            ll += mx
            if t == 0 and defect != "first_step_not_skipped":
                continue
            s00, s01, s10, s11 = a00 * b0, a01 * b1, a10 * b0, a11 * b1
            n00, n01 = m00 * s00 + m01 * s10, m00 * s01 + m01 * s11
            n10, n11 = m10 * s00 + m11 * s10, m10 * s01 + m11 * s11
            r = 1.0 / (n00 + n01 + n10 + n11)
            m00, m01, m10, m11 = n00 * r, n01 * r, n10 * r, n11 * r
        pm[p] = (m00, m01, m10, m11)
        acc[p][8] = ll
    # 2. hmm_cuts: alpha forwards, beta backwards
    edge = [None] * (P + 1)
    v0, v1 = pi0 * B0[0], pi1 * B1[0]
    edge[0] = (v0, v1)
    s = v0 + v1
    v0, v1 = v0 / s, v1 / s
    for p in range(P - 1):
        M = pm[p]
        w0, w1 = v0 * M[0] + v1 * M[2], v0 * M[1] + v1 * M[3]
        s = w0 + w1
        v0, v1 = w0 / s, w1 / s
        edge[p + 1] = (v0, v1)
    edgeB = [None] * (P + 1)
    v0 = v1 = 0.5
    edgeB[P] = (v0, v1)
    for p in range(P - 1, 0, -1):
        M = pm[p]
        w0, w1 = M[0] * v0 + M[1] * v1, M[2] * v0 + M[3] * v1
        s = w0 + w1
        v0, v1 = w0 / s, w1 / s
        edgeB[p] = (v0, v1)
    # 3. hmm_forward_walk
    A0, A1 = [0.0] * n, [0.0] * n
    for p in range(P):
        a, b = cut[p], cut[p + 1]
        ll = 0.0
        t = a
        if p == 0:
            s = edge[0][0] + edge[0][1]
            ll += math.log(s)
            v0, v1 = edge[0][0] / s, edge[0][1] / s
            A0[0], A1[0] = v0, v1
            t = 1
        else:
            q = p
            if defect == "cut_from_neighbour":
                q = p + 1 if p + 1 < P else p - 1
                q = max(q, 1)
            v0, v1 = edge[q]
        prod, held = 1.0, 0
        first = p > 0
        while t < b:
            w0, w1 = (v0 * a00 + v1 * a10) * B0[t], (v0 * a01 + v1 * a11) * B1[t]
            s = w0 + w1
            r = 1.0 / s
            if not (first and defect == "first_scale_left_out"):
                prod *= s
            first = False
            held += 1
            if held == 4 or prod < 1e-200:
                ll += math.log(prod)
                prod, held = 1.0, 0
            v0, v1 = w0 * r, w1 * r
            A0[t], A1[t] = v0, v1
            t += 1
        if defect != "flush_drops_held":
            ll += math.log(prod)
        acc[p][9] = ll
    # 4. hmm_backward_walk (pieces in ascending order: when piece p runs, the last window of piece p - 1 already holds a posterior)
    for p in range(P):
        a, b = cut[p], cut[p + 1]
        be0, be1 = edgeB[p + 2] if (defect == "beta_edge_of_next" and p + 2 <= P) else edgeB[p + 1]
        g0s = g1s = gx0 = gx1 = x00 = x01 = x10 = x11 = 0.0
        for t in range(b - 1, a - 1, -1):
            g0, g1 = A0[t] * be0, A1[t] * be1
            gr = 1.0 / (g0 + g1)
            g0 *= gr
            g1 *= gr
            fwd_prev = (A0[t - 1], A1[t - 1]) if t > 0 else None
            A0[t], A1[t] = g0, g1
            xt = x[t]
            g0s += g0; g1s += g1; gx0 += g0 * xt; gx1 += g1 * xt      # noqa: E702
            if t == 0:
                break
            b0, b1 = B0[t] * be0, B1[t] * be1
            if t > a or defect == "xi_from_posterior":
                p0, p1 = fwd_prev
            else:
                p0, p1 = edge[p]
            e00, e01, e10, e11 = p0 * a00 * b0, p0 * a01 * b1, p1 * a10 * b0, p1 * a11 * b1
            er = 1.0 / (e00 + e01 + e10 + e11)
            x00 += e00 * er; x01 += e01 * er; x10 += e10 * er; x11 += e11 * er      # noqa: E702
            nb0, nb1 = a00 * b0 + a01 * b1, a10 * b0 + a11 * b1
            br = 1.0 / (nb0 + nb1)
            be0, be1 = nb0 * br, nb1 * br
        acc[p][0:8] = [g0s, g1s, gx0, gx1, x00, x01, x10, x11]
    S = [_reduce_rows([acc[p][k] for p in range(P)]) for k in range(10)]
    post = np.stack((np.array(A0), np.array(A1)), axis=1)
    return post, np.array(S[:8]), S[8] + S[9]


# ------------------------------------------------------------------------------------------------------------------- Viterbi
VIT_STEPS = 256           # frisk_hmm_gpu::VIT_STEPS


def viterbi(x, model, steps=VIT_STEPS):
    """hmm_vit_pieces, hmm_vit_cuts and hmm_vit_backtrack for ONE sequence, operation for operation in float64: list of states."""
    x = [float(v) for v in np.asarray(x, dtype=np.float64)]
    n = len(x)
    if n == 0:
        return []
    ninf = float("-inf")
    lg = lambda v: math.log(v) if v > 0 else ninf      # noqa: E731
    mu, cv = [float(v) for v in model["means"]], [float(v) for v in model["covars"]]
    lc = [math.log(v) for v in cv]
    ls = [lg(float(v)) for v in model["start"]]
    (t00, t01), (t10, t11) = ((lg(float(v)) for v in row) for row in model["trans"])
    ll = lambda xt, j: -0.5 * ((LOG2PI + lc[j]) + (xt - mu[j]) * (xt - mu[j]) / cv[j])      # noqa: E731
    pa = list(range(0, n, steps))
    pb = [min(a + steps, n) for a in pa]
    back, M = [0] * n, []
    for k, (a, b) in enumerate(zip(pa, pb)):
        e0, e1 = ll(x[a], 0), ll(x[a], 1)
        r = [[ls[0] + e0, ls[1] + e1], [ls[0] + e0, ls[1] + e1]] if k == 0 else [[t00 + e0, t01 + e1], [t10 + e0, t11 + e1]]
        for t in range(a + 1, b):
            l0, l1 = ll(x[t], 0), ll(x[t], 1)
            bits = 0
            for e in (0, 1):
                c00, c10, c01, c11 = r[e][0] + t00, r[e][1] + t10, r[e][0] + t01, r[e][1] + t11
                k0, k1 = int(c10 > c00), int(c11 > c01)
                bits |= (k0 | (k1 << 1)) << (2 * e)
                r[e] = [(c10 if k0 else c00) + l0, (c11 if k1 else c01) + l1]
            back[t] = bits
        M.append(r)
    K = len(pa)
    choice, endst, entry = [0] * K, [0] * K, [0] * K
    v0, v1 = M[0][0]
    for k in range(1, K):
        mx = max(v0, v1)
        if mx > ninf:
            v0, v1 = v0 - mx, v1 - mx
        q = M[k]
        c00, c10, c01, c11 = v0 + q[0][0], v1 + q[1][0], v0 + q[0][1], v1 + q[1][1]
        h0, h1 = int(c10 > c00), int(c11 > c01)
        choice[k] = h0 | (h1 << 1)
        v0, v1 = (c10 if h0 else c00), (c11 if h1 else c01)
    st = int(v1 > v0)
    for k in range(K - 1, -1, -1):
        endst[k] = st
        entry[k] = (choice[k] >> st) & 1 if k > 0 else 0
        st = entry[k]
    path = [0] * n
    for k, (a, b) in enumerate(zip(pa, pb)):
        cur, sh = endst[k], 2 * entry[k]
        for t in range(b - 1, a, -1):
            path[t] = cur
            cur = (back[t] >> (sh + cur)) & 1
        path[a] = cur
    return path
