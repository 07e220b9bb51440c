#!/usr/bin/env python3
"""Compare the device assembly of two builds of the library, unit by unit.

    tools/isa_compare.py PARENT_OBJDIR CANDIDATE_OBJDIR

Both directories are object directories of scale-letkf_amd/Makefile (lib/obj, lib/obj_prof, ...): the build leaves
<unit>-hip-amdgcn-amd-amdhsa-gfx950.s of every unit there.  Two files count as the same when they are equal after this
normalisation and nothing more: lines that contain __hip_cuid_ are dropped (a hash of the source text), and everything from
a ';' to the end of a line is dropped (comments carry the mangled names of inlined functions, which change when a helper is
renamed or moved).  Instructions, labels, register numbers, .amdhsa_* lines and kernel symbol names are compared as they are.
Prints one line per unit; exit status 1 if a unit differs or exists on one side only.  For a refactor of device code that
must not move the compiler's output: build the parent in a copy of its tree, the candidate in place, and compare."""
import glob
import os
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def normalised(path):
    with open(path, errors="replace") as f:
        return [ln.split(";", 1)[0].rstrip() for ln in f if "__hip_cuid_" not in ln]


def units(objdir):
    return {os.path.basename(p)[: -len(SUFFIX)]: p for p in glob.glob(os.path.join(objdir, "*" + SUFFIX))}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = units(sys.argv[1]), units(sys.argv[2])
    if not a and not b:
        sys.exit("no *%s in either directory" % SUFFIX)
    bad = 0
    for u in sorted(set(a) | set(b)):
        if u not in a or u not in b:
            print("%-16s only in %s" % (u, sys.argv[1] if u in a else sys.argv[2]))
            bad += 1
            continue
        x, y = normalised(a[u]), normalised(b[u])
        if x == y:
            print("%-16s same (%d lines)" % (u, len(x)))
            continue
        bad += 1
        first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print("%-16s DIFFERENT (%d / %d lines), first at normalised line %d:" % (u, len(x), len(y), first + 1))
        print("    parent:    %s" % (x[first] if first < len(x) else "<end>"))
        print("    candidate: %s" % (y[first] if first < len(y) else "<end>"))
    print("%d units, %d different" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
