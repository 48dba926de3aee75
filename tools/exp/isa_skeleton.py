#!/usr/bin/env python3
"""(CPU) inventory of the per-window skeleton of the K = 8 / 4-bit plain bulk kernel: the device assembly of one kernel cut at its
barriers, the nine unrolled copies of the scoring loop (tools/exp/isa_copies.py's blocks) left out, and the instructions of every
stage counted by kind - VALU, SALU (s_nop, s_waitcnt and branches apart), LDS, VMEM, scratch.  The counts are of the stage's code -
every path through it, an instruction on a rare branch like one on the straight line -, so two builds are compared stage by stage
as a reader of the assembly would; what a window issues is the profile's business (SQ_INSTS_VALU / SQ_INSTS_SALU per window).
Usage: python tools/exp/isa_skeleton.py FILE.s [ROLE]   (ROLE: 0 = kmin an argument, the default; 4 = compiled for kmin = 1)"""
import re, sys
asm, role = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "0")
kern = '_Z12scan8_kernelILi8ELi256ELi20ELi4ELi64ELi3ELb0ELi%sELb0EEv10ScanParams' % role
L = open(asm).read().split('\n')
a = next(i for i, l in enumerate(L) if l.startswith(kern + ':'))
b = next(i for i in range(a, len(L)) if 's_endpgm' in L[i])
K = [l for l in L[a:b] if re.match(r'\s+[a-z]', l) and not re.match(r'\s+\.', l)]
bars = [-1] + [i for i, l in enumerate(K) if 's_barrier' in l] + [len(K)]
print("%s: %d instructions, %d barriers" % (kern, len(K), len(bars) - 2))
print("%-8s %6s %6s %6s %6s %6s %6s %6s %6s" % ("segment", "valu", "salu", "branch", "wait", "nop", "lds", "vmem", "scratch"))
tot = [0] * 8
for n, (lo, hi) in enumerate(zip(bars, bars[1:])):
    B = K[lo + 1:hi]
    c = lambda p: sum(1 for l in B if re.match(r'\s+' + p, l))
    loop = c('v_frexp_mant_f64') >= 10          # (holds the copies of the scoring loop: its blocks are isa_copies.py's)
    if loop:
        # drop the straight-line blocks with >= 10 positions; keep what surrounds them (dispatch, sums' butterfly, orphan loading)
        cuts = [0] + [i for i, l in enumerate(B) if re.match(r'\s+s_(c?branch|setpc)', l)] + [len(B)]
        keep = []
        for x, y in zip(cuts, cuts[1:]):
            blk = B[x:y]
            if sum(1 for l in blk if 'v_frexp_mant_f64' in l) < 10: keep += blk
        B = keep
    row = [c('v_'), c(r's_(?!nop|waitcnt|c?branch|setpc|barrier)'), c(r's_(c?branch|setpc)'), c('s_waitcnt'), c('s_nop'), c('ds_'),
           c('(global|buffer|flat)_'), c('scratch_')]
    tot = [t + r for t, r in zip(tot, row)]
    print("%-8s %6d %6d %6d %6d %6d %6d %6d %6d%s" % (("b%d..b%d" % (n, n + 1),) + tuple(row) + ("   (around the scoring loop's copies)" if loop else "",)))
print("%-8s %6d %6d %6d %6d %6d %6d %6d %6d" % (("all",) + tuple(tot)))
