#!/usr/bin/env python3
"""Serialised loads of every kernel of a .hip unit: the vector-memory loads (global_ / buffer_ / flat_ / scratch_load_*)
whose next vector-memory-relevant instruction is a full `s_waitcnt vmcnt(0)`, i.e. nothing else is put in flight between
the load and the wait for it.  Vector-memory-relevant: every global_ / buffer_ / flat_ / scratch_ instruction and every
s_waitcnt that names vmcnt; the instruction stream is read in program order, labels and branches are not followed.
Compiled with kernel_regs.py's flags.

usage: tools/kernel_waits.py unit.hip [...] [--check NAME-SUBSTRING] [--md]
Prints the kernels that have any; --check exits 1 when a kernel whose name contains the substring has one."""
import re
import subprocess
import sys
import tempfile
import os

from kernel_regs import FLAGS

VMEM = re.compile(r"^\s+(global|buffer|flat|scratch)_(\w+)")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*)")


def assembly(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        extra = os.environ.get("PCR_EXTRA_FLAGS", "").split()
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + [src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def short(symbol):
    name = subprocess.run(["c++filt", symbol], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(anonymous namespace\)::|pcrhip::", "", name).split("(")[0].replace("void ", "")


def waits(text):
    """[(kernel, vector-memory loads, loads followed by a full wait)] for every kernel of the assembly"""
    kernels = set(re.findall(r"^\s+\.amdhsa_kernel\s+(\S+)", text, re.M))
    rows, name, loads, bad, pending = [], None, 0, 0, False
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in kernels:
            name, loads, bad, pending = m.group(1), 0, 0, False
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            rows.append((short(name), loads, bad))
            name = None
            continue
        code = line.split(";")[0]
        v, w = VMEM.match(code), WAIT.match(code)
        if v:
            pending = v.group(2).startswith("load")
            loads += pending
        elif w and "vmcnt" in w.group(1):
            if pending and re.search(r"vmcnt\(0\)", w.group(1)):
                bad += 1
            pending = False
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    check = None
    if "--check" in args:
        i = args.index("--check")
        check = args[i + 1]
        del args[i:i + 2]
    md = "--md" in args
    units = [a for a in args if a != "--md"]
    failed = 0
    print("| unit | kernel | loads | followed by vmcnt(0) |\n|---|---|---|---|" if md else
          f"{'kernel':84s} loads  followed by vmcnt(0)")
    for unit in units:
        for name, loads, bad in waits(assembly(unit)):
            if bad:
                print(f"| {os.path.basename(unit)} | `{name}` | {loads} | {bad} |" if md else f"{name[:84]:84s} {loads:5d}  {bad:5d}")
                if check is not None and check in name:
                    failed += 1
    if check is not None:
        print(f"--check {check}: " + ("FAILED" if failed else "ok"))
    sys.exit(1 if failed else 0)
