"""Length-matched null distributions for region scores - host specification of the device generator and of the draws.

`generate()` restates csrc/null_kernels.h (frisk_seq_null) in numpy and produces the same bytes, as synth.py does for
synth_kernel.h.  The definition:

  * digits  : A, T, G, C = 0..3, first base most significant, as everywhere
  * table   : the chain of order r reads the SYMMETRIC counts of order r + 1 of a finalised profile.  For context c in [0, 4^r):
              cum_b(c) = sum_{b' <= b} sym_{r+1}[4c + b'] as uint64, T(c) = cum_3(c)
  * blocks  : a sequence is cut into blocks of BLOCK = 4096 bases, each independent.  A block starts from
              state = mix(seed ^ mix((seq << 40) ^ blk ^ (12 << 56))), ctx = 0.  One step: state += GOLDEN, x = mix(state);
              T(ctx) == 0: b = x >> 62;  otherwise u = mulhi64(x, T(ctx)), b = (u >= cum_0) + (u >= cum_1) + (u >= cum_2);
              then ctx = ((ctx << 2) | b) & (4^r - 1).  The first BURN = 64 steps are discarded (nine times the longest context of
              7 bases: part of the definition, not a tuned value); step 64 + t writes "ATGC"[b] at position 4096 blk + t
  * output  : uppercase only, no N.  Every base is a pure function of (profile, order, seed, sequence index, position), so a
              sequence is a prefix of any longer one with the same index

`host_draws()` chooses the slices of the host that the "host" null scores, and `stats()` turns the null KLDs of one length into the
columns of python -m frisk_amd.regions --null.
"""
import math

import numpy as np

from .engine import table_offset
from .synth import GOLDEN, _mix

BLOCK = 4096
BURN = 64
SALT_BLOCK = 12             # (synth.py's unit hashes use salts 1 .. 11)
SALT_HOST = 13
MAX_BATCH = (1 << 63) - 64  # padded positions a batch layout can address (int64, rounded up to 32)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_U64 = (1 << 64) - 1
_LETTERS = np.frombuffer(b"ATGC", dtype=np.uint8)


def mix_int(z):
    """synth_mix on a Python integer."""
    z &= _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def mulhi64(x, t):
    """High 64 bits of the 128-bit product of two uint64 arrays (__umul64hi)."""
    x = np.asarray(x, dtype=np.uint64)
    t = np.asarray(t, dtype=np.uint64)
    xl, xh, tl, th = x & _M32, x >> _S32, t & _M32, t >> _S32
    lh, hl = xl * th, xh * tl
    mid = ((xl * tl) >> _S32) + (lh & _M32) + (hl & _M32)
    return xh * th + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def cum_table(sym, kmin, order):
    """(4^order, 4) uint64: the running sums of the profile's symmetric counts of order `order` + 1, one row per context."""
    off = table_offset(kmin, order + 1)
    rows = np.asarray(sym[off:off + 4 ** (order + 1)], dtype=np.int64).astype(np.uint64).reshape(-1, 4)
    return np.cumsum(rows, axis=1, dtype=np.uint64)


def _blocks(cum, order, seed, seq, blk):
    """(n, BLOCK) uint8: block blk[i] of sequence seq[i], all of them stepped together."""
    seq = np.asarray(seq, dtype=np.uint64)
    blk = np.asarray(blk, dtype=np.uint64)
    seed = np.uint64(int(seed) & _U64)
    mask = np.int64(4 ** order - 1)
    state = _mix(seed ^ _mix((seq << np.uint64(40)) ^ blk ^ (np.uint64(SALT_BLOCK) << np.uint64(56))))
    ctx = np.zeros(seq.size, dtype=np.int64)
    out = np.zeros((seq.size, BLOCK), dtype=np.uint8)
    with np.errstate(over="ignore"):
        for t in range(-BURN, BLOCK):
            state = state + GOLDEN
            x = _mix(state)
            row = cum[ctx]
            total = row[:, 3]
            u = mulhi64(x, total)
            b = (u >= row[:, 0]).astype(np.int64) + (u >= row[:, 1]) + (u >= row[:, 2])
            b = np.where(total == 0, (x >> np.uint64(62)).astype(np.int64), b)
            ctx = ((ctx << 2) | b) & mask
            if t >= 0:
                out[:, t] = _LETTERS[b]
    return out


def generate_batch(sym, kmin, order, seed, lens):
    """[bytes] - the batch frisk_seq_null(lens, seed, order) makes resident under the finalised profile `sym` (orders from kmin)."""
    lens = [int(n) for n in lens]
    cum = cum_table(sym, kmin, order)
    nblk = [(n + BLOCK - 1) // BLOCK for n in lens]
    seq = np.repeat(np.arange(len(lens)), nblk)
    blk = np.concatenate([np.arange(n) for n in nblk]) if seq.size else np.zeros(0, np.int64)
    flat = _blocks(cum, order, seed, seq, blk)
    out, at = [], 0
    for n, k in zip(lens, nblk):
        out.append(flat[at:at + k].reshape(-1)[:n].tobytes())
        at += k
    return out


def generate(sym, kmin, order, seed, seq_index, length):
    """bytes of sequence `seq_index` of a null batch, `length` bases."""
    length = int(length)
    if length <= 0:
        return b""
    nblk = (length + BLOCK - 1) // BLOCK
    flat = _blocks(cum_table(sym, kmin, order), order, seed, np.full(nblk, int(seq_index)), np.arange(nblk))
    return flat.reshape(-1)[:length].tobytes()


def batch_fits(draws, longest):
    """Can a batch of `draws` sequences of `longest` bases be laid out (one PAD behind each, int64 positions)?"""
    return int(draws) < (1 << 31) and int(draws) * (int(longest) + 1) <= MAX_BATCH


def host_draws(lens, length, draws, seed):
    """[(scaffold, offset)] * draws: the slices of `length` bases of the host that form its null at this length.  Over the scaffolds
    with len >= length, in batch order, there are total = sum(len - length + 1) start positions; draw j takes the one of index
    mulhi64(mix(seed ^ mix((length << 24) ^ j ^ (13 << 56))), total).  [] when no scaffold is long enough."""
    scaf, off = host_draw_arrays(lens, length, draws, seed)
    return list(zip(scaf.tolist(), off.tolist()))


def host_draw_arrays(lens, length, draws, seed):
    """host_draws as two int64 arrays (scaffold, offset), empty when no scaffold is long enough."""
    length = int(length)
    seed = int(seed) & _U64
    keep = [(s, int(n) - length + 1) for s, n in enumerate(lens) if int(n) >= length]
    total = sum(k for _, k in keep)
    if length < 1 or total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    key = np.uint64(((length << 24) ^ (SALT_HOST << 56)) & _U64) ^ np.arange(int(draws), dtype=np.uint64)
    idx = mulhi64(_mix(np.uint64(seed) ^ _mix(key)), np.uint64(total)).astype(np.int64)
    ends = np.cumsum([k for _, k in keep], dtype=np.int64)
    at = np.searchsorted(ends, idx, side="right")
    scaf = np.asarray([s for s, _ in keep], dtype=np.int64)[at]
    off = idx - (ends[at] - np.asarray([k for _, k in keep], dtype=np.int64)[at])
    return scaf, off


def stats(kld, null):
    """(nullN, nullMean, nullSD, excess, z, p) of one region's KLD against the valid null KLDs of its length; None stands for `.`.
    mean = fsum(v) / n; SD = sqrt(fsum((v - mean)^2) / (n - 1)), None for n < 2; excess = KLD - mean; z = excess / SD, None without
    an SD or with SD 0; p = (1 + #{v >= KLD}) / (1 + n): ties count against the region.  n = 0: all None."""
    v = [float(x) for x in null]
    n = len(v)
    if n == 0:
        return None, None, None, None, None, None
    kld = float(kld)
    mean = math.fsum(v) / n
    sd = math.sqrt(math.fsum((x - mean) ** 2 for x in v) / (n - 1)) if n >= 2 else None
    excess = kld - mean
    z = excess / sd if sd else None
    p = (1 + sum(1 for x in v if x >= kld)) / float(1 + n)
    return n, mean, sd, excess, z, p
