#!/usr/bin/env python3
"""Compare the gfx950 kernels of two device-assembly listings.

    hipcc $(HIPFLAGS) -S --cuda-device-only -o old.s old.hip      (one listing per source file)
    tools/kernel_asm_diff.py old.s new_a.s [new_b.s ...] [--rename OLD=NEW]

Every kernel of old.s is looked up in the new listings and compared in two respects: the instruction
stream between its label and its .Lfunc_end, and its .amdhsa_kernel descriptor block.  Comments are
dropped and the per-file function numbers in local labels (.LBB<n>_, .LJTI<n>_, .Lfunc_end<n>) are
rewritten to a constant.  --rename rewrites a substring of old.s's symbol names first (a kernel whose
template arguments changed).  For kernels that differ, the descriptor lines that differ are printed.
Exit status 1 when a kernel is missing or differs.
"""
import re
import sys


def kernels(text):
    """name -> (body lines, descriptor lines)"""
    text = re.sub(r"\.(LBB|LJTI|Lfunc_end|Lfunc_begin)\d+", r".\1", text)
    lines = [re.sub(r"\s*;.*$", "", ln).strip() for ln in text.split("\n")]
    lines = [ln for ln in lines if ln]
    out = {}
    for i, ln in enumerate(lines):
        if not ln.startswith(".amdhsa_kernel "):
            continue
        name = ln.split()[1]
        desc = lines[i + 1:lines.index(".end_amdhsa_kernel", i)]
        b = lines.index(name + ":")
        e = next(k for k in range(b, len(lines)) if lines[k].startswith(".Lfunc_end"))
        out[name] = (lines[b + 1:e], desc)
    return out


def main(argv):
    renames = []
    while "--rename" in argv:
        k = argv.index("--rename")
        renames.append(argv[k + 1].split("=", 1))
        del argv[k:k + 2]
    if len(argv) < 3:
        sys.exit(__doc__)
    old_text = open(argv[1]).read()
    for a, b in renames:
        old_text = old_text.replace(a, b)
    old = kernels(old_text)
    new = {}
    for p in argv[2:]:
        new.update(kernels(open(p).read()))
    bad = 0
    for name in sorted(old):
        if name not in new:
            print(f"MISSING    {name}")
            bad += 1
            continue
        same_body, same_desc = old[name][0] == new[name][0], old[name][1] == new[name][1]
        if same_body and same_desc:
            continue
        bad += 1
        print(f"DIFFERENT  {name}: body {'same' if same_body else 'differs'} "
              f"({len(old[name][0])} -> {len(new[name][0])} lines), descriptor {'same' if same_desc else 'differs'}")
        od, nd = dict(l.split(None, 1) for l in old[name][1]), dict(l.split(None, 1) for l in new[name][1])
        for k in od:
            if od[k] != nd.get(k):
                print(f"    {k}: {od[k]} -> {nd.get(k)}")
    extra = sorted(set(new) - set(old))
    for name in extra:
        print(f"NEW        {name}")
    print(f"{len(old)} kernels in {argv[1]}, {len(new)} in the new listings, {len(old) - bad} identical, {bad} not")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
