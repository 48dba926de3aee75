#!/usr/bin/env python3
"""Wall-clock of the projection's k-mer vectors on the synthetic generator (Engine.synth): n windows of w bases at orders a..b,
  (a) projection.symmetricCounts on the windows' slices - load into a fresh Engine, debug scan with one window per sequence, the
      forward count dump to the host, fold and divide row by row in Python;
  (b) projection.windowVectors on the resident batch (csrc/kvec_kernels.h) - count, fold and divide on the device.
Each with a split: (a) kernel = the scan kernels' event time, copy = the rest of the scan call (the count dump's way to the host),
python = the fold loop; (b) kernel = frisk_last_kernel_ms(3), copy = the rest of the call (allocation, X's way to the host).
The two routes' rows are compared bit for bit on a sample.

Without --step this is the driver: every step is a child process under its own `timeout`, one after the other, and the first
failure stops the run.  One process uses the GPU at a time.

    python tools/kvec_timing.py [--n 20000] [--w 5000] [--orders 1 6] [--limit 600] [--device 0]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def batch(a, engine):
    """one scaffold of n * w synthetic bases (no N, no soft-masking: every window passes the 30 % rule); its windows as ranges"""
    engine.synth([a.n * a.w], 7, island_frac=0.05)
    start = np.arange(a.n, dtype=np.int64) * a.w
    return np.zeros(a.n, np.int32), start, start + a.w


def step_a(a):
    from frisk_amd import Engine
    from frisk_amd.projection import proportions_from_forward, symmetricCounts
    with Engine(a.orders[0], a.orders[1], a.device) as e:
        _s, start, _e = batch(a, e)
        whole = e.read_seq(0).decode("ascii")
    seqs = [whole[p:p + a.w] for p in start.tolist()]
    t0 = time.perf_counter()
    _labels, X = symmetricCounts([(str(i), s) for i, s in enumerate(seqs)], a.orders[0], a.orders[1], device=a.device)
    total = time.perf_counter() - t0
    # the same steps once more, one by one (what symmetricCounts does inside)
    with Engine(a.orders[0], a.orders[1], a.device) as e:
        t0 = time.perf_counter()
        e.load(seqs)
        load = time.perf_counter() - t0
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        t0 = time.perf_counter()
        res = e.scan(max(a.w, 2), 1, scaffolds_all=True, debug=True)
        scan = time.perf_counter() - t0
        kernel = e.kernel_ms(0) / 1e3
    t0 = time.perf_counter()
    rows = [proportions_from_forward(res.counts[i], a.orders[0], a.orders[1]) for i in range(len(seqs))]
    python = time.perf_counter() - t0
    assert all(rows[i].tolist() == X[i].tolist() for i in range(0, len(seqs), max(1, len(seqs) // 50)))
    np.save(os.path.join(a.scratch, "kvec_a_sample.npy"), X[::max(1, a.n // 200)])
    return {"route": "symmetricCounts", "total_s": total, "load_s": load, "kernel_s": kernel, "copy_s": scan - kernel, "python_s": python}


def step_b(a):
    from frisk_amd import Engine
    from frisk_amd.projection import windowVectors
    with Engine(a.orders[0], a.orders[1], a.device) as e:
        seq, start, stop = batch(a, e)
        windowVectors(e, seq[:8], start[:8], stop[:8], a.orders[0], a.orders[1])        # (first launch: code object load)
        t0 = time.perf_counter()
        X = windowVectors(e, seq, start, stop, a.orders[0], a.orders[1])
        total = time.perf_counter() - t0
        kernel = e.kernel_ms(3) / 1e3
    sample = os.path.join(a.scratch, "kvec_a_sample.npy")
    same = bool(np.array_equal(np.load(sample), X[::max(1, a.n // 200)])) if os.path.exists(sample) else None
    return {"route": "windowVectors", "total_s": total, "kernel_s": kernel, "copy_s": total - kernel, "rows_equal_route_a": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--w", type=int, default=5000)
    ap.add_argument("--orders", type=int, nargs=2, default=[1, 6])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--limit", type=int, default=600, help="seconds a step may take")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build"))
    ap.add_argument("--step", choices=["a", "b"], default=None)
    a = ap.parse_args()
    os.makedirs(a.scratch, exist_ok=True)
    if a.step:
        print(json.dumps(dict({"a": step_a, "b": step_b}[a.step](a), n=a.n, w=a.w, orders=a.orders)), flush=True)
        return 0
    out = []
    for step in ("a", "b"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(a.n), "--w", str(a.w),
               "--orders", str(a.orders[0]), str(a.orders[1]), "--device", str(a.device), "--scratch", a.scratch]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print("step %s ended with status %d: stopping" % (step, p.returncode), file=sys.stderr)
            return p.returncode
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    ra, rb = out
    print("| route | total s | kernel s | copy s | Python s |\n|---|---|---|---|---|")
    print("| (a) symmetricCounts on slices | %.3f | %.3f | %.3f | %.3f |" % (ra["total_s"], ra["kernel_s"], ra["copy_s"], ra["python_s"]))
    print("| (b) windowVectors on the resident batch | %.3f | %.3f | %.3f | - |" % (rb["total_s"], rb["kernel_s"], rb["copy_s"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
