#!/usr/bin/env python3
"""Are two builds of a kernel translation unit the same device code (no GPU needed)?
usage: tools/cmp_device_asm.py A.s B.s, each from   hipcc <the Makefile's HIPFLAGS> --offload-device-only -S -o X.s csrc/<unit>.hip
Compares the two assembly files per kernel symbol; the kernels may come in any order.  Masked: the __hip_cuid_<hex> symbol (a hash of the translation unit) and the function's ordinal in the
file that local labels carry (.LBB<n>_k, .Lfunc_end<n>, .LJTI<n>_k, .LCPI<n>_k).  Every line of both files is attributed
either to a kernel (code, kernel descriptor, resource comments, metadata entry) or to the rest, which is compared as well."""
import re, sys

def norm(s):
    s = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", s)
    s = re.sub(r"(\.L|\b)(BB|JTI|CPI)\d+_", r"\1\2_", s)  # (labels, and the comments that name them)
    s = re.sub(r"[ \t]+;", " ;", s)  # (the padding in front of a comment depends on the label's width)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s)

def split(path):
    lines = open(path).read().split("\n")
    begin = re.compile(r"^\t\.protected\t(\S+)\s+; -- Begin function")
    starts = []
    for i, l in enumerate(lines):
        m = begin.match(l)
        if m:
            starts.append((i - 1 if lines[i - 1].startswith(("\t.section\t.text", "\t.text")) else i, m.group(1)))
    md = lines.index("amdhsa.kernels:")
    parts, rest = {}, lines[:starts[0][0]]
    for k, (s, name) in enumerate(starts):
        if k + 1 < len(starts):
            e = starts[k + 1][0]
        else:  # the last kernel: through its resource comments
            e = next(i for i in range(s, md) if "; -- End function" in lines[i]) + 1
            while e < md and (not lines[e].strip() or lines[e].startswith(("\t.set ", ";")) or ".AMDGPU.csdata" in lines[e]):
                e += 1
            rest += lines[e:md]
        assert name not in parts, name
        parts[name] = [norm("\n".join(lines[s:e]))]
    # the metadata: one entry of amdhsa.kernels per kernel, then the file's trailer
    i = md + 1
    cur = None
    while i < len(lines) and (lines[i].startswith("  - .agpr_count:") or lines[i].startswith("    ")):
        if lines[i].startswith("  - "):
            cur = []
            entries = cur
            parts.setdefault(None, []).append(cur)
        cur.append(lines[i])
        i += 1
    for ent in parts.pop(None, []):
        name = next(re.search(r"\.name:\s+(\S+)", l).group(1) for l in ent if ".name:" in l)
        parts[name].append(norm("\n".join(ent)))
    rest += lines[md:md + 1] + lines[i:]
    return parts, norm("\n".join(rest))

a, ra = split(sys.argv[1]); b, rb = split(sys.argv[2])
bad = 0
if sorted(a) != sorted(b):
    print("symbol sets differ:", sorted(set(a) ^ set(b))); bad = 1
for k in sorted(set(a) & set(b)):
    if len(a[k]) != 2 or a[k] != b[k]:
        print("DIFFERS:", k, [len(x) for x in a[k]], [len(x) for x in b[k]]); bad = 1
if ra != rb:
    print("the lines outside the kernels differ"); bad = 1
print("%s: %d kernel symbols, %s" % (sys.argv[2], len(a), "DIFFERENT" if bad else "identical per symbol"))
sys.exit(bad)
