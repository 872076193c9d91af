#!/usr/bin/env python3
"""Kernel resources and opcode counts of csrc/tt_trace.hip and csrc/tt_shadow.hip, one tree against another (the
form of profiles/r*/*/registers.txt). Each side is a directory holding, per file F of tt_trace and tt_shadow, F.s and
F.remarks from

    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only -Rpass-analysis=kernel-resource-usage -o DIR/F.s csrc/F.hip 2> DIR/F.remarks

Usage: tools/kernel_registers.py PARENT_DIR NEW_DIR > registers.txt. Exit status 1 if a kernel outside
tt_trace_leaf_kernel differs in resources or in any opcode count."""
import collections
import re
import sys

FIELDS = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "ScratchSize [bytes/lane]": "ScratchSize",
          "Occupancy [waves/SIMD]": "Occupancy", "SGPRs Spill": "SGPRsSpill", "VGPRs Spill": "VGPRsSpill",
          "LDS Size [bytes/block]": "LDS"}


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def opcodes(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), collections.Counter())
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
        m = re.match(r"^\t([a-z][a-z0-9_]+)\b", line)
        if cur is not None and m and not line.startswith("\t."):
            cur[m.group(1)] += 1
    return out


def main():
    parent, new = sys.argv[1], sys.argv[2]
    bad = 0
    for f in ("tt_trace", "tt_shadow"):
        rp, rn = resources(f"{parent}/{f}.remarks"), resources(f"{new}/{f}.remarks")
        op, on = opcodes(f"{parent}/{f}.s"), opcodes(f"{new}/{f}.s")
        for k in sorted(rn):
            a, b = op.get(k, {}), on.get(k, {})
            diff = [f"{o}: {a.get(o, 0)} -> {b.get(o, 0)}" for o in sorted(set(a) | set(b)) if a.get(o, 0) != b.get(o, 0)]
            same = rp.get(k) == rn[k] and not diff
            bad += (not same) and "tt_trace_leaf_kernel" not in k
            print(("same " if same else "DIFF ") + k)
            print(f"    parent {rp.get(k)}")
            print(f"    new    {rn[k]}")
            print("    opcodes: " + (", ".join(diff) if diff else "identical"))
            print(f"    instructions: {sum(a.values())} -> {sum(b.values())}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
