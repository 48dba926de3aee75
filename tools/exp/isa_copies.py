#!/usr/bin/env python3
"""(CPU) device assembly of the units that hold the 4-bit narrow-counter kernels (scan8_launch4.hip, scan8_launch41.hip); for the K = 8 / 4-bit bulk kernels (plain and SIDE, each with kmin as an argument and compiled for kmin = 1) the copies of the scoring loop:
instructions per position and scratch accesses in each.  Usage: python tools/exp/isa_copies.py [extra -D flags]
(--asm FILE: read that device assembly instead of compiling.)  Behind the runs of positions, the straight-line copies one by one: every
basic block that scores at least half a lane's positions (the unrolled copies of the K = 8 scoring loop are one block each), with its
instruction counts by kind for the whole block."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC, HIP_FLAGS, CSRC
os.makedirs(os.path.join(ROOT, "build/isa"), exist_ok=True)
flags = sys.argv[1:]
given = flags.index("--asm") if "--asm" in flags else -1
if given >= 0:
    asms, flags = [flags[given + 1]], flags[:given] + flags[given + 2:]
else:
    asms = [os.path.join(ROOT, "build/isa/%s.s" % u) for u in ("scan8_launch4", "scan8_launch41")]
    for out in asms:
        subprocess.run([HIPCC] + HIP_FLAGS + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, os.path.basename(out)[:-2] + ".hip")],
                       check=True, stderr=subprocess.DEVNULL)
L = [l for f in asms for l in open(f).read().split('\n')]
for tag, kern in (('plain', '_Z12scan8_kernelILi8ELi256ELi20ELi4ELi64ELi3ELb0ELi0ELb0EEv10ScanParams'),
                  ('side', '_Z12scan8_kernelILi8ELi256ELi20ELi4ELi64ELi3ELb0ELi0ELb1EEv10ScanParams'),
                  ('plain_kmin1', '_Z12scan8_kernelILi8ELi256ELi20ELi4ELi64ELi3ELb0ELi4ELb0EEv10ScanParams'),
                  ('side_kmin1', '_Z12scan8_kernelILi8ELi256ELi20ELi4ELi64ELi3ELb0ELi4ELb1EEv10ScanParams')):
    if not any(l.startswith(kern + ':') for l in L): continue        # (--asm: one unit's kernels)
    a = next(i for i, l in enumerate(L) if l.startswith(kern + ':'))
    b = next(i for i in range(a, len(L)) if 's_endpgm' in L[i])
    K = L[a:b]
    open(os.path.join(ROOT, 'build/isa/%s.s' % tag), 'w').write('\n'.join(K))
    bars = [i for i, l in enumerate(K) if 's_barrier' in l]
    seg = max(zip(bars, bars[1:]), key=lambda ab: ab[1] - ab[0])
    r = [i for i in range(*seg) if 'v_frexp_mant_f64' in K[i]]
    gaps = sorted(y - x for x, y in zip(r, r[1:])); med = gaps[len(gaps) // 2]
    labels = [i for i in range(*seg) if re.match(r'\.LBB\d+_\d+:', K[i])]
    runs = []; cur = [r[0]]
    for x, y in zip(r, r[1:]):
        if y - x > 2.2 * med: runs.append(cur); cur = [y]
        else: cur.append(y)
    runs.append(cur)
    for run in runs:
        lo, hi = run[0], run[-1]
        n = max(1, len(run) - 1)
        c = lambda p: sum(1 for l in K[lo:hi] if re.match(r'\s+' + p, l))
        print(tag, 'copy at %5d..%5d: %2d positions; per position: valu %.1f salu %.1f lds %.1f vmem %.1f; scratch ops %d, labels %d' % (
            lo, hi, len(run), c('v_') / n, c('s_') / n, c('ds_') / n, c('(global|buffer|flat)_') / n, c('scratch_'), sum(1 for l in labels if lo < l < hi)))
    # the straight-line copies: basic blocks (label to label / branch) of the scoring stage with >= 10 positions
    cuts = sorted(set([seg[0]] + labels + [i for i in range(*seg) if re.match(r'\s+s_(c?branch|setpc)', K[i])] + [seg[1]]))
    for lo, hi in zip(cuts, cuts[1:]):
        B = K[lo:hi]
        c = lambda p: sum(1 for l in B if re.match(r'\s+' + p, l))
        npos = c('v_frexp_mant_f64')
        if npos < 10: continue
        print(tag, 'block at %5d..%5d: %2d positions; in all: valu %d (f64 %d, cndmask %d) salu %d (s_nop %d) lds %d vmem %d (stores %d); scratch ops %d, v_readlane/writelane %d' % (
            lo, hi, npos, c('v_'), c(r'v_\w+_f64'), c('v_cndmask'), c('s_'), c('s_nop'), c('ds_'), c('(global|buffer|flat)_'), c('(global|buffer|flat)_store'),
            c('scratch_'), c('v_(read|write)lane')))
