#!/usr/bin/env python3
"""(CPU) how far ahead of its use the K = 8 scoring loop requests a position's logarithm-table entry: in the hot copy of the plain 4-bit
bulk kernel (the straight-line block with the fewest vector instructions among those that score a lane's 20 positions), for every
ds_read_b128 of the table, the vector instructions issued between the read and the s_waitcnt that drains it (LDS operations return
in order: a wait for lgkmcnt(n) drains all but the last n requested).
Usage: python tools/exp/isa_logtab_gap.py [build/isa/plain.s] [table offset, default 15072]   (the file: tools/exp/isa_copies.py writes it)"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build/isa/plain.s")
offset = sys.argv[2] if len(sys.argv) > 2 else "15072"
K = open(path).read().split("\n")
cuts = sorted(set([0, len(K)] + [i for i, l in enumerate(K) if re.match(r"\.LBB\d+_\d+:", l) or re.match(r"\s+s_(c?branch|setpc|barrier)", l)]))
blocks = [(lo, hi) for lo, hi in zip(cuts, cuts[1:]) if sum("v_frexp_mant_f64" in l for l in K[lo:hi]) >= 20]
lo, hi = min(blocks, key=lambda b: sum(1 for l in K[b[0]:b[1]] if re.match(r"\s+v_", l)))
pending, gaps, valu = [], [], 0           # requests not yet drained: (is the table's, vector instructions issued before it)
for l in K[lo:hi]:
    if re.match(r"\s+v_", l):
        valu += 1
    elif re.match(r"\s+(ds_|s_load|s_buffer_load)", l):
        pending.append((bool(re.match(r"\s+ds_read_b128 .*offset:%s\b" % offset, l)), valu))
    else:
        m = re.match(r"\s+s_waitcnt.*lgkmcnt\((\d+)\)", l)
        if m:
            keep = int(m.group(1))
            done, pending = pending[:len(pending) - keep], pending[len(pending) - keep:] if keep else []
            gaps += [valu - at for mine, at in done if mine]
print("hot copy at %d..%d: %d table reads; vector instructions between a read and the wait that drains it: %s" % (lo, hi, len(gaps), gaps))
if gaps:
    print("min %d, median %d, mean %.1f" % (min(gaps), sorted(gaps)[len(gaps) // 2], sum(gaps) / len(gaps)))
