#!/usr/bin/env python3
"""(GPU) profile kernel time (HIP events) of prebuilt libraries, alternating, two rounds: usage prof_ab.py [--shapes K:SHAPE,...] lib1.so lib2.so ...
A shape is kmax and `shard` (the 410 Mb bench shard) or `c5` (the whole 3.29 Gb genome of that bench).  The default takes each form of
phase A once: K = 8 on the shard (two halves) and on the whole genome (one pass), K = 6 (one table) and K = 10 (global table) on the shard.
raw_sum is the sum of the raw profile: a library that counts something else shows at once."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD = r'''
import sys, json
sys.path.insert(0, %r)
from frisk_amd import Engine, synth
LENS = {"shard": lambda: synth.c5_shard_lens(8, 0), "c5": lambda: [n for r in range(8) for n in synth.c5_shard_lens(8, r)]}
out = {}
for shape in sys.argv[1].split(","):
    kmax, label = shape.split(":")
    with Engine(1, int(kmax)) as e:
        e.synth(LENS[label](), seed=0xC5, island_frac=0.02, n_frac=0.07, lower_frac=0.0)
        ts = []
        for _ in range(6):
            e.profile_reset(); e.profile_add(); ts.append(e.kernel_ms(1)); e.profile_finalize()
        out[shape] = {"profile_ms_best": round(min(ts), 4), "raw_sum": int(e.profile_raw().sum())}
print(json.dumps(out))
''' % ROOT
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="8:shard,8:c5,6:shard,10:shard")
ap.add_argument("libs", nargs="+")
args = ap.parse_args()
for rnd in range(2):
    for lib in args.libs:
        o = subprocess.run([sys.executable, "-c", CHILD, args.shapes], env=dict(os.environ, FRISK_HIP_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=300)
        print(os.path.basename(lib), o.stdout.strip() or o.stderr[-300:], flush=True)
        if o.returncode:            # nothing more on a device that a library may have faulted
            sys.exit("%s: exit %d" % (lib, o.returncode))
