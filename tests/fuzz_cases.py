"""The case generator of the differential fuzz (tests/test_gpu_fuzz.py), shared with the CPU calibration of the KLD precision
bound (tests/test_kld_precision_cpu.py): geometry, word sizes, flags and sequence make-up (N runs, soft-masked runs, IUPAC
letters, low-complexity runs, tiny scaffolds) drawn from a numpy Generator.  Changing it changes the cases both draw."""
import numpy as np


def random_case(rng, kmax_hi=8):
    """One case of the differential fuzz: a dict of kmin, kmax, w, inc, seqs (bytes), mask_host, scaffolds_all, rip."""
    kmax = int(rng.integers(1, kmax_hi + 1))
    kmin = int(rng.integers(1, kmax + 1))
    w = int(rng.choice([37, 64, 100, 333, 512, 1000, 2048, 2049, 5000, 5121, 8192, 8193, 12000, 66000]))
    inc = max(1, int(w * rng.choice([0.05, 0.2, 0.5, 0.9, 1.0, 1.6])))
    seqs = []
    for _ in range(int(rng.integers(1, 6))):
        n = int(rng.choice([0, 5, w // 2, w, w + 1, 2 * w + 3, 3 * w, 7 * w + int(rng.integers(0, w))]))
        p = rng.dirichlet([2, 2, 2, 2])
        s = rng.choice(np.frombuffer(b"ATGC", dtype=np.uint8), size=n, p=p)
        for _ in range(int(rng.integers(0, 6))):
            if n == 0:
                break
            a = int(rng.integers(0, n))
            ln = int(rng.choice([1, 2, 7, 8, 9, 40, w // 3 + 1]))
            kind = rng.integers(0, 4)
            if kind == 0:
                s[a:a + ln] = ord("N")
            elif kind == 1:
                s[a:a + ln] |= 0x20                           # soft-masked
            elif kind == 2:
                s[a:a + ln] = rng.choice(np.frombuffer(b"RYKMnrx-*", dtype=np.uint8), size=len(s[a:a + ln]))
            else:
                s[a:a + ln] = s[a] if a < n else ord("A")      # a low-complexity run (big counts)
        seqs.append(s.tobytes())
    return dict(kmin=kmin, kmax=kmax, w=w, inc=inc, seqs=seqs, mask_host=bool(rng.integers(0, 2)),
                scaffolds_all=bool(rng.integers(0, 2)), rip=bool(rng.integers(0, 2)) and kmin <= 2 <= kmax)
