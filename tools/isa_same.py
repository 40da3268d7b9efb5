#!/usr/bin/env python3
"""Are two builds' gfx950 kernels the same machine code?  (refactor check, no GPU)

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize \
          --cuda-device-only -S -o X.s csrc/X.hip        # per file, both trees (as isa_mix.py)
    tools/isa_same.py OLD NEW                            # two .s files or two directories of them

Kernels are matched by symbol across all the files of a side, so code may move
between translation units.  Per kernel three texts are compared: the body
(label to .Lfunc_end), the .amdhsa_kernel block and the amdhsa.kernels
metadata entry (registers, LDS, scratch, arguments); device objects
(__constant__ / __device__ tables) are compared by symbol as well.  Local
labels lose their per-file function index first; comments and __hip_cuid_*
lines are dropped.  Text comparison only.  Exit status 1 on any difference.
"""
import glob
import os
import re
import sys

LOCAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+")


def norm(lines):
    """without comments (they carry block numbers too), blank lines and __hip_cuid_ lines"""
    out = [LOCAL.sub(r".\1", ln if '"' in ln else ln.split(";")[0]).rstrip() for ln in lines if "__hip_cuid_" not in ln]
    return [ln for ln in out if ln]


def parse(path):
    """{symbol: {part: [lines]}} of every .s file under path"""
    out = {}
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]
    for f in files:
        L = open(f).read().split("\n")
        for i, ln in enumerate(L):
            m = re.match(r"\s*\.type\s+([\w$.]+),@(function|object)", ln)
            if m and "__hip_cuid_" not in ln:
                name, kind = m.groups()
                a = next(j for j in range(i, len(L)) if L[j].startswith(name + ":"))
                end = (lambda s: s.startswith(".Lfunc_end")) if kind == "function" else (
                    lambda s: s.strip().startswith(".size") and name + "," in s)
                b = next(j for j in range(a, len(L)) if end(L[j]))
                out.setdefault(name, {})["body" if kind == "function" else "object"] = norm(L[a:b + 1])
            m = re.match(r"\s*\.amdhsa_kernel\s+([\w$.]+)", ln)
            if m:
                b = next(j for j in range(i, len(L)) if ".end_amdhsa_kernel" in L[j])
                out.setdefault(m.group(1), {})["descriptor"] = norm(L[i:b + 1])
        if "amdhsa.kernels:" in L:   # the metadata's kernel list: entries start with "  - "
            a = L.index("amdhsa.kernels:") + 1
            b = next(j for j in range(a, len(L)) if L[j] and not L[j].startswith(" "))
            starts = [j for j in range(a, b) if L[j].startswith("  - ")] + [b]
            for s, e in zip(starts, starts[1:]):
                name = next(x.split(":", 1)[1].strip() for x in L[s:e] if x.strip().startswith(".name:"))
                out.setdefault(name, {})["metadata"] = norm(L[s:e])
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "only in " + ("OLD" if name in old else "NEW")
        else:
            diff = [p for p in sorted(set(old[name]) | set(new[name])) if old[name].get(p) != new[name].get(p)]
            verdict = "differs: " + ", ".join(diff) if diff else "same"
        bad += verdict != "same"
        kind = "kernel" if "descriptor" in old.get(name, new.get(name)) else "object"
        print(f"{verdict:28s} {kind:7s} {name}")
    print(f"{len(set(old) | set(new))} symbols, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
