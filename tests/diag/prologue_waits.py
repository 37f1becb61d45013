#!/usr/bin/env python3
"""Diagnostic: how many full waits does a kernel pay between its entry and a given instruction?

Reads gfx9 assembly (`hipcc --offload-arch=gfx950 --cuda-device-only -S`) and, for every kernel whose (mangled) name matches a regular
expression, walks the instructions from the kernel's label along the laid-out path - conditional branches fall through (the compiler
lays the working path out that way and sends the early exits forward), unconditional ones are followed - up to the first instruction
that matches `--until`, counting the `s_waitcnt` that drain a counter: `lgkmcnt(0)` (scalar loads: kernel arguments, scalars) or
`vmcnt(0)` (vector loads).  Each is one memory round trip the instructions behind it cannot overlap with.

    python tests/diag/prologue_waits.py pgo_ml_kernels.s 'ml_cg_comp_pcg_kernelILi5ELb0' --until 'global_load_'
    python tests/diag/prologue_waits.py pgo_ml_kernels.s 'ml_spmv_pcg_kernel' --until 'global_load_dword$'

Prints one JSON object per kernel: name, waits, the wait instructions with their line numbers, the line the walk ended at.
tests/test_pcg_prologue_isa.py holds the small-graph PCG pair to its bounds with count_waits()."""
import argparse
import json
import re
import sys

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_FULL_WAIT = re.compile(r"\b(lgkmcnt|vmcnt)\(0\)")


def kernels(lines, name_re):
    """(name, index of the label line) of every function label that matches"""
    pat = re.compile(name_re)
    out = []
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m and not m.group(1).startswith(".") and pat.search(m.group(1)):
            out.append((m.group(1), i))
    return out


def count_waits(lines, start, until_re):
    """walks from line index `start`; returns (waits [(line number, text)], line number of the first `until` instruction or None)"""
    until = re.compile(until_re)
    labels = {}
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m:
            labels[m.group(1)] = i
    waits, i, seen = [], start + 1, set()
    while i < len(lines) and i not in seen:
        seen.add(i)
        ins = lines[i].split(";")[0].strip()
        if not ins or _LABEL.match(ins) or ins.startswith("."):
            i += 1
            continue
        op = ins.split()[0]
        if until.search(op):
            return waits, i + 1
        if op == "s_endpgm":
            return waits, None
        if op == "s_waitcnt" and _FULL_WAIT.search(ins):
            waits.append((i + 1, ins))
        if op == "s_branch":
            tgt = ins.split()[1]
            if tgt not in labels:
                return waits, None
            i = labels[tgt]
            continue
        i += 1
    return waits, None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="regular expression on the mangled kernel name")
    ap.add_argument("--until", default="global_load_", help="regular expression on the mnemonic the walk ends at (default: any global load)")
    a = ap.parse_args()
    lines = open(a.asm).read().splitlines()
    found = kernels(lines, a.kernel)
    if not found:
        print("no kernel matches %r" % a.kernel, file=sys.stderr)
        return 1
    for name, at in found:
        waits, end = count_waits(lines, at, a.until)
        print(json.dumps({"kernel": name, "waits": len(waits), "at": waits, "until_line": end}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
