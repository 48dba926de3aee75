#!/bin/bash
# usage: build_variant.sh <name> [-D flags...]  ->  build/ab/<name>.so (+ register / scratch report of the scan kernels in build/ab/<name>.res.txt)
name=$1; shift
mkdir -p build/ab
python3 -c "import sys, __graft_entry__ as g; g.build_hip(force=True, extra_flags=sys.argv[1:] + ['-Rpass-analysis=kernel-resource-usage'], out='build/ab/$name.so')" "$@" 2> build/ab/$name.res.txt
rc=$?
grep -E "error" -A3 build/ab/$name.res.txt | head -20
exit $rc
