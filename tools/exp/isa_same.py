#!/usr/bin/env python3
"""(CPU) do two trees build the same device code?  Usage: python tools/exp/isa_same.py <other tree> [this tree]
Compiles every frisk_amd/csrc/*.hip of both trees to device assembly (one file per unit, units side by side, flags of
__graft_entry__.HIP_FLAGS), cuts the assembly per kernel - from the kernel's label to its .Lfunc_end, plus its .amdhsa_kernel
descriptor -, drops comments and .loc lines, replaces the numbers in local labels that depend on a kernel's place in its unit
(.LBB<n>_, .Ltmp<n>, ...) and requires the same set of kernel names, each kernel in one unit only, and equal text per kernel.
Plain text equality between two builds: a refactor that moves kernels between units must leave every one of them as it was.
An assembly file newer than its tree's sources is reused (build/isa/same/ of this tree)."""
import glob, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC, HIP_FLAGS


def device_asm(tree, tag):
    csrc = os.path.join(tree, "frisk_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa", "same", tag)
    os.makedirs(out, exist_ok=True)
    deps = glob.glob(os.path.join(csrc, "*")) + glob.glob(os.path.join(tree, "include", "*.h"))
    newest = max(os.path.getmtime(d) for d in deps)
    flags = [f for f in HIP_FLAGS if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include"), "-I" + csrc]
    units = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    asms = [os.path.join(out, os.path.basename(u) + ".s") for u in units]

    def one(u, s):
        if not (os.path.exists(s) and os.path.getmtime(s) > newest):
            subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "-o", s, u], check=True, stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(max_workers=min(len(units), 16)) as pool:
        list(pool.map(one, units, asms))
    return asms


def kernels(asms):
    """kernel name -> (unit, normalised text)"""
    found = {}
    for s in asms:
        L = open(s).read().split("\n")
        names = [l.split()[1] for l in L if l.lstrip().startswith(".amdhsa_kernel ")]
        for name in names:
            a = next(i for i, l in enumerate(L) if l.startswith(name + ":"))
            b = next(i for i in range(a, len(L)) if L[i].startswith(".Lfunc_end"))
            d0 = next(i for i, l in enumerate(L) if l.lstrip().startswith(".amdhsa_kernel " + name))
            d1 = next(i for i in range(d0, len(L)) if l_is_end(L[i]))
            text = []
            for l in L[a:b] + L[d0:d1]:
                l = l.split(";")[0].rstrip()
                if not l or l.lstrip().startswith(".loc"):
                    continue
                text.append(re.sub(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b", lambda m: ".L" + m.group(1) + (m.group(2) or ""), l))
            if name in found:
                sys.exit("kernel %s is in two units: %s and %s" % (name, found[name][0], s))
            found[name] = (os.path.basename(s), "\n".join(text))
    return found


def l_is_end(l):
    return l.lstrip().startswith(".end_amdhsa_kernel")


def main():
    other = os.path.abspath(sys.argv[1])
    this = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT
    A, B = kernels(device_asm(other, "a")), kernels(device_asm(this, "b"))
    missing, added = sorted(set(A) - set(B)), sorted(set(B) - set(A))
    differ = sorted(k for k in set(A) & set(B) if A[k][1] != B[k][1])
    for k in missing: print("only in %s: %s (%s)" % (other, k, A[k][0]))
    for k in added: print("only in %s: %s (%s)" % (this, k, B[k][0]))
    for k in differ: print("differs: %s (%s / %s)" % (k, A[k][0], B[k][0]))
    units = lambda K: len(set(u for u, _ in K.values()))
    print("isa_same: %d kernels in %d unit(s) against %d kernels in %d unit(s): %d missing, %d added, %d differ" % (
        len(A), units(A), len(B), units(B), len(missing), len(added), len(differ)))
    sys.exit(1 if missing or added or differ else 0)


if __name__ == "__main__":
    main()
