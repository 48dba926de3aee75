#!/usr/bin/env python3
"""(GPU) same-box A/B of prebuilt libraries on the geometries beside the flagship: usage ab_shapes.py [rounds] lib1.so lib2.so ... - for
each library in turn, `rounds` times over: HIP-event time of the scan kernels on the bench shard (410 Mb), best of 6, at
K = 8 w = 5000 inc = 1007 (the general copies of the scoring loop), K = 8 w = 2048 inc = 400 (8 positions per lane), K = 7 and K = 6 at
w = 5000 inc = 1000, plus a checksum of the rows.  A child that does not end cleanly ends the run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD = r'''
import sys, json
sys.path.insert(0, %r)
from frisk_amd import Engine, synth
out = {}
for label, kmax, w, inc in (("k8_inc1007", 8, 5000, 1007), ("k8_w2048", 8, 2048, 400), ("k7", 7, 5000, 1000), ("k6", 6, 5000, 1000)):
    with Engine(1, kmax) as e:
        e.synth(synth.c5_shard_lens(8, 0), seed=0xC5, island_frac=0.02, n_frac=0.07, lower_frac=0.0)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        ts = []
        for _ in range(6):
            r = e.scan(w, inc, pinned=True); ts.append(e.kernel_ms(0))
        out[label] = {"best": round(min(ts), 4), "last": round(ts[-1], 3), "kld_sum": float(r.kld[r.kept].sum()), "stat": e.scan_stat()[:3]}
print(json.dumps(out))
'''
args = sys.argv[1:]
rounds = int(args.pop(0)) if args and args[0].isdigit() else 2
for rnd in range(rounds):
    for lib in args:
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=dict(os.environ, FRISK_HIP_LIB=os.path.abspath(lib)), capture_output=True, text=True)
        print(os.path.basename(lib), out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr[-400:], flush=True)
        if out.returncode != 0:
            sys.exit("child ended with %d" % out.returncode)
