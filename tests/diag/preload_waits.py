#!/usr/bin/env python3
"""Diagnostic: which kernels have their leading arguments preloaded into SGPRs, and how many full waits stand between a kernel's REAL
entry and its first load of an operand?

Reads gfx9 assembly (`hipcc --offload-arch=gfx950 --cuda-device-only -S`, with the flags of csrc/Makefile) like prologue_waits.py,
whose walk it extends (same path: conditional branches fall through, unconditional ones are followed).  For every kernel whose
(mangled) name matches the regular expression it reports

    preload_sgprs   `.amdhsa_user_sgpr_kernarg_preload_length` of the kernel descriptor: SGPRs the command processor fills from the
                    head of the kernel-argument segment before the waves start (0 = nothing is preloaded)
    waits           full waits (`s_waitcnt lgkmcnt(0)` / `vmcnt(0)`) from the real entry up to the first load of an OPERAND - any
                    vector load, or a scalar load whose base is not the kernel-argument segment pointer
    fetch_loads     scalar loads of the kernel-argument segment on that stretch (they run beside the operand load when waits = 0)

A kernel with preloaded arguments starts with a compatibility prologue (for firmware that does not preload: it loads the same SGPRs,
waits, and branches to the next 256-byte boundary); firmware that preloads enters at that boundary.  The walk starts there.  It looks
at argument loads and waits and at nothing else.

    python tests/diag/preload_waits.py pgo_ml_kernels.s 'ml_spmv_pcg_kernel|ml_cg_comp_pcg_kernelILi5ELb0'
    python tests/diag/preload_waits.py pgo_lm_kernels.s 'lm_head_kernel|lm_tail_kernel|eval_lm_kernel|hessian_lm_kernel'

Prints one JSON object per kernel.  tests/test_pcg_preload_isa.py holds ml_spmv_pcg_kernel to its numbers with walk()."""
import argparse
import importlib.util
import json
import os
import re
import sys

_spec = importlib.util.spec_from_file_location("prologue_waits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "prologue_waits.py"))
_pw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_pw)

_FULL_WAIT = re.compile(r"\b(lgkmcnt|vmcnt)\(0\)")
_VLOAD = re.compile(r"^(global|flat|buffer|scratch)_load_")
_SLOAD = re.compile(r"^s_(buffer_)?load_")


def descriptor(lines, name):
    """the `.amdhsa_*` directives of kernel `name` as {directive: int}"""
    out, inside = {}, False
    for ln in lines:
        t = ln.strip()
        if t.startswith(".amdhsa_kernel "):
            inside = t.split()[1] == name
        elif t.startswith(".end_amdhsa_kernel"):
            if inside:
                return out
        elif inside and t.startswith(".amdhsa_"):
            f = t.split()
            try:
                out[f[0]] = int(f[1], 0)
            except (IndexError, ValueError):
                pass
    return out


def kernarg_pair(desc):
    """the SGPR pair that holds the kernel-argument segment pointer: user SGPRs are handed out in a fixed order"""
    at = 4 * desc.get(".amdhsa_user_sgpr_private_segment_buffer", 0) + 2 * desc.get(".amdhsa_user_sgpr_dispatch_ptr", 0) \
        + 2 * desc.get(".amdhsa_user_sgpr_queue_ptr", 0)
    return "s[%d:%d]" % (at, at + 1)


def real_entry(lines, start, preloaded):
    """index of the line the waves start at: the kernel's label, or - with preloaded arguments - the aligned block behind the
    compatibility prologue's branch"""
    if not preloaded:
        return start
    labels = {}
    for i, ln in enumerate(lines):
        m = _pw._LABEL.match(ln)
        if m:
            labels[m.group(1)] = i
    for i in range(start + 1, min(start + 40, len(lines))):
        ins = lines[i].split(";")[0].strip()
        if ins.startswith("s_branch"):
            return labels.get(ins.split()[1], start)
        if ins.startswith("s_endpgm"):
            break
    return start


def walk(lines, start, karg):
    """from line index `start`: (full waits [(line number, text)], kernel-argument loads [(line number, text)], line number of the
    first operand load or None)"""
    labels = {}
    for i, ln in enumerate(lines):
        m = _pw._LABEL.match(ln)
        if m:
            labels[m.group(1)] = i
    waits, fetch, i, seen = [], [], start + 1, set()
    while i < len(lines) and i not in seen:
        seen.add(i)
        ins = lines[i].split(";")[0].strip()
        if not ins or _pw._LABEL.match(ins) or ins.startswith("."):
            i += 1
            continue
        op = ins.split()[0]
        if _VLOAD.match(op):
            return waits, fetch, i + 1
        if _SLOAD.match(op):
            base = [x.strip() for x in ins[len(op):].split(",")][1]
            if base != karg:
                return waits, fetch, i + 1
            fetch.append((i + 1, ins))
        if op == "s_endpgm":
            return waits, fetch, None
        if op == "s_waitcnt" and _FULL_WAIT.search(ins):
            waits.append((i + 1, ins))
        if op == "s_branch":
            tgt = ins.split()[1]
            if tgt not in labels:
                return waits, fetch, None
            i = labels[tgt]
            continue
        i += 1
    return waits, fetch, None


def report(lines, name, at):
    desc = descriptor(lines, name)
    n_pre = desc.get(".amdhsa_user_sgpr_kernarg_preload_length", 0)
    entry = real_entry(lines, at, n_pre > 0)
    waits, fetch, end = walk(lines, entry, kernarg_pair(desc))
    return {"kernel": name, "preload_sgprs": n_pre, "entry_line": entry + 1, "waits": len(waits), "at": waits,
            "fetch_loads": len(fetch), "first_operand_load_line": end}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="regular expression on the mangled kernel name")
    a = ap.parse_args()
    lines = open(a.asm).read().splitlines()
    found = _pw.kernels(lines, a.kernel)
    if not found:
        print("no kernel matches %r" % a.kernel, file=sys.stderr)
        return 1
    for name, at in found:
        print(json.dumps(report(lines, name, at)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
