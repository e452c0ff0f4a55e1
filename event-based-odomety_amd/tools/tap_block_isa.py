#!/usr/bin/env python3
"""Opcode histogram of the tap blocks of k_eval3<true> in csrc/ebo_kernels.s (`make asm`): the basic blocks (label to
label / branch) that hold at least 40 ds_add_u64 (the scatter's interior block) or 40 ds_read_b64 (the gather's), and
the kernel's register counts.  A reading for profiles/, not a gate.

    python3 tools/tap_block_isa.py csrc/ebo_kernels.s [kernel-name-substring]
"""
import collections
import re
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_eval3ILb1"
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % want, l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    blocks, cur = [], []
    for l in lines[start + 1:end]:
        t = l.strip()
        if re.match(r"^\.LBB\d+_\d+:", t):
            blocks.append(cur)
            cur = []
            continue
        m = re.match(r"^([vs]_|ds_|global_|scratch_|buffer_|flat_)\w+", t)
        if m:
            cur.append(m.group(0))
            if m.group(0).startswith(("s_cbranch", "s_branch", "s_setpc")):
                blocks.append(cur)
                cur = []
    blocks.append(cur)
    total = collections.Counter(op for b in blocks for op in b)
    valu = sum(n for op, n in total.items() if op.startswith("v_"))
    print("kernel *%s*: %d instructions, %d VALU, %d basic blocks" % (want, sum(total.values()), valu, len(blocks)))
    for what in ("ds_add_u64", "ds_read_b64"):
        for b in blocks:
            h = collections.Counter(b)
            if h[what] >= 40:
                print("-- block with %d %s: %d instructions, %d VALU" % (h[what], what, len(b), sum(n for op, n in h.items() if op.startswith("v_"))))
                for op, n in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])):
                    print("   %4d %s" % (n, op))
    meta = next(i for i in range(end, len(lines)) if re.match(r"^\s+\.name:\s+\w*%s" % want, lines[i]))
    first = max(i for i in range(end, meta + 1) if re.match(r"^\s+- \.", lines[i]))
    last = next((i for i in range(meta + 1, len(lines)) if re.match(r"^\s+- \.[a-z_]+:\s", lines[i]) and not lines[i].startswith("      ")), len(lines))
    for l in lines[first:last]:
        if re.search(r"\.(vgpr_count|vgpr_spill_count|sgpr_count|sgpr_spill_count|private_segment_fixed_size):", l):
            print(l.strip().lstrip("- "))


if __name__ == "__main__":
    main()
