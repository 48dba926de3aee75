#!/bin/bash
# usage: build_tune.sh <out.so> [extra -D flags...]
out=$1; shift
cd "$(dirname "$0")/../.."
python3 -c "import sys, __graft_entry__ as g; g.build_hip(force=True, extra_flags=['-DFRISK_TUNE'] + sys.argv[2:] + ['-Rpass-analysis=kernel-resource-usage'], out=sys.argv[1])" "$out" "$@" 2> ${out%.so}.res.txt
rc=$?
grep -E "error" ${out%.so}.res.txt | head
python3 - "${out%.so}.res.txt" <<'PY'
import re,sys
txt=open(sys.argv[1]).read()
blocks=re.split(r"remark: [^\n]*Function Name: ", txt)
for b in blocks[1:]:
    name=b.split("\n")[0]
    if 'scan8' not in name and 'scan_kernel' not in name: continue
    g=lambda k: re.search(k+r": (\d+)", b)
    vals=[(g(k).group(1) if g(k) else '?') for k in ["VGPRs","SGPRs","ScratchSize \[bytes/lane\]","Occupancy \[waves/SIMD\]"]]
    print(name[:60], "vgpr/sgpr/scratch/occ", vals)
PY
exit $rc
