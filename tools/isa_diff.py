#!/usr/bin/env python
"""Compare the gfx950 kernels of two device-assembly files (hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include
--cuda-device-only -S <file>.hip): for every kernel symbol present in both, the instruction text between its label and the end of
the function (its last s_endpgm) and its .amdhsa_* resource block must be identical.  Exit status 1 when a shared kernel differs.
    python tools/isa_diff.py before.s after.s"""
import re
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    body, res = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", lines[i])
        if m and i and ".type\t%s,@function" % m.group(1) in "\n".join(lines[max(0, i - 6):i]):
            j = i + 1
            while ".amdhsa_kernel" not in lines[j]:   # (a kernel may hold several s_endpgm: all text up to its resource block)
                j += 1
            # comments dropped; basic-block labels are .LBB<function ordinal>_<n>: the ordinal moves when a kernel leaves the file
            body[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", l)) for l in lines[i + 1:j]]
            i = j
        m = re.match(r"^\s*\.amdhsa_kernel (\w+)", lines[i])
        if m:
            j = i + 1
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            res[m.group(1)] = [l.strip() for l in lines[i + 1:j]]
            i = j
        i += 1
    return body, res


def main(a, b):
    ba, ra = kernels(a)
    bb, rb = kernels(b)
    bad = 0
    print("%s: %d kernels, %s: %d kernels" % (a, len(ra), b, len(rb)))
    for k in sorted(set(ra) ^ set(rb)):
        print("only in %s: %s" % (a if k in ra else b, k))
    for k in sorted(set(ra) & set(rb)):
        same_i, same_r = ba[k] == bb[k], ra[k] == rb[k]
        vg = [l.split()[-1] for l in ra[k] if "next_free_vgpr" in l or "group_segment_fixed_size" in l or "private_segment_fixed_size" in l]
        print("%-62s %6d instruction lines %s, resources %s (scratch/lds/vgpr %s)" % (
            k, len(ba[k]), "IDENTICAL" if same_i else "DIFFER", "IDENTICAL" if same_r else "DIFFER", "/".join(vg)))
        bad += not (same_i and same_r)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
