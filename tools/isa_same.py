#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    make -C tipe-raytracer_amd asm          # at each commit: rt_kernels.s
    tools/isa_same.py OLD.s NEW.s [--allow-reordered] [--allow-new]

Comments are stripped and the function-index part of local labels
(.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>) is normalised; kernels are matched by
mangled symbol.  For every kernel the instruction text and the
.amdhsa_kernel descriptor block (VGPRs, SGPRs, LDS and scratch bytes, ...)
must be identical: exit status 0.

--allow-reordered (source refactors that may commute an operand or move an
instruction): a kernel may differ when its descriptor block, its instruction
count and its multiset of opcode mnemonics are all identical.  Those kernels
are listed with their differing lines; anything beyond that class fails.

--allow-new (a change that adds kernels): symbols present only in NEW.s are
listed as new and do not fail; a symbol missing from NEW.s still does.
"""
import collections
import difflib
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")


def norm(line):
    line = line.split(";", 1)[0].strip()
    return LABEL.sub(lambda m: "." + m.group(1), line)


def kernels(path):
    """{symbol: (body lines, descriptor lines)} of the .amdhsa_kernel symbols."""
    body, desc = {}, {}
    cur = dcur = None
    for raw in open(path):
        line = norm(raw)
        if not line:
            continue
        if dcur is not None:
            if line == ".end_amdhsa_kernel":
                dcur = None
            else:
                desc[dcur].append(line)
            continue
        if line.startswith(".amdhsa_kernel "):
            dcur = line.split()[1]
            desc[dcur] = []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                body[cur].append(line)
            continue
        m = re.match(r"([A-Za-z_$][\w$.]*):$", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            body[cur] = []
    return {k: (body.get(k, []), d) for k, d in desc.items()}


def insns(lines):
    return [l for l in lines if not l.startswith(".") and not l.endswith(":")]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    allow = "--allow-reordered" in sys.argv[1:]
    allow_new = "--allow-new" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    bad = 0
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    if gone or (added and not allow_new):
        bad += 1
    for k in gone:
        print("only in %s: %s" % (args[0], k))
    for k in added:
        print("%s %s: %s" % ("NEW in" if allow_new else "only in", args[1], k))
    same, reordered = 0, []
    for k in sorted(set(old) & set(new)):
        (b0, d0), (b1, d1) = old[k], new[k]
        if b0 == b1 and d0 == d1:
            same += 1
            continue
        i0, i1 = insns(b0), insns(b1)
        ops0 = collections.Counter(l.split()[0] for l in i0)
        ops1 = collections.Counter(l.split()[0] for l in i1)
        why = []
        if d0 != d1:
            why.append("descriptor differs")
        if len(i0) != len(i1):
            why.append("instruction count %d -> %d" % (len(i0), len(i1)))
        if ops0 != ops1:
            why.append("opcode multiset differs")
        if why or not allow:
            bad += 1
            print("DIFFERENT %s: %s" % (k, ", ".join(why) or "instruction text differs"))
            for l in difflib.unified_diff(d0, d1, "old descriptor", "new descriptor", lineterm="", n=0):
                print("    " + l)
        else:
            reordered.append(k)
            print("REORDERED %s (same descriptor, instruction count %d, opcode multiset)" % (k, len(i0)))
        if not why:
            for l in difflib.unified_diff(b0, b1, "old", "new", lineterm="", n=0):
                print("    " + l)
    print("%d kernels in %s, %d in %s: %d identical, %d reordered, %d failing"
          % (len(old), args[0], len(new), args[1], same, len(reordered), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
