"""What the region scorer's timing tools share (ranges_timing.py, panel_timing.py, explain_timing.py, null_timing.py): the synthetic
batch - 16 scaffolds of 4 Mb from Engine.synth, 1 % N, 5 % soft-masked -, the three workloads on it and the median of repeated
measurements.
  grid    every candidate window of w = 5000, i = 1000 passed as ranges
  mixed   50 000 ranges with seeded log-uniform lengths between 300 and 30 000 bases
  long    the scaffolds themselves (the global-scratch form)
"""
import statistics

import numpy as np

W, INC = 5000, 1000
BATCH_SEED = 7
SYNTH = dict(island_frac=0.02, n_frac=0.01, lower_frac=0.05)


def add_arguments(ap):
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scaffolds", type=int, default=16)
    ap.add_argument("--scaffold-len", type=int, default=4000000)


def synth_batch(e, lens, seed=BATCH_SEED):
    e.synth(lens, seed, **SYNTH)


def own_profile(e):
    e.profile_reset(); e.profile_add(); e.profile_finalize()


def grid_of(scan):
    """The windows of a scan as ranges - a jumpback window by its slice."""
    jump = (scan.status & 4) != 0
    return scan.seq_index.copy(), np.where(jump, scan.start, scan.start - 1), scan.stop.copy()


def log_uniform_lengths(rng, n):
    return np.exp(rng.uniform(np.log(300), np.log(30000), n)).astype(np.int64)


def mixed(n_scaffolds, scaffold_len, n=50000):
    rng = np.random.default_rng(11)
    ln = log_uniform_lengths(rng, n)
    s = rng.integers(0, n_scaffolds, n).astype(np.int32)
    a0 = (rng.random(n) * (scaffold_len - ln)).astype(np.int64)
    return s, a0, a0 + ln


def whole(lens):
    return np.arange(len(lens), dtype=np.int32), np.zeros(len(lens), np.int64), np.asarray(lens, np.int64)


def median_ms(fn, ms, repeats):
    """Median over `repeats` calls of fn, after one warm-up, of ms() read behind each - of fn's own value where ms is None."""
    fn()
    out = []
    for _ in range(repeats):
        v = fn()
        out.append(v if ms is None else ms())
    return statistics.median(out)
