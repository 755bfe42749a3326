#!/usr/bin/env python3
"""Device code of two trees, kernel by kernel: compiles every csrc/*.hip unit of this tree and of OTHER (a checkout of the
commit to compare against) to gfx950 assembly with kernel_regs.py's flags and reports every function whose instruction
stream or code-object metadata differs, and every symbol only one side has.  For host-side refactors: the answer must be
"identical".  usage: tools/kernel_diff.py OTHER_TREE [unit.hip ...]        exit status 1 when anything differs

Ignored: the __hip_cuid_* symbol, .file / .ident lines, comments, and the function index inside local labels
(.LBB<idx>_<n>), which moves when kernels are instantiated in a different order."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

from kernel_regs import ROOT, flags

CSRC = os.path.join("pointcloud-raster_amd", "csrc")
META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "kernarg_segment_size")


def assembly(root, unit):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags(root) + [os.path.join(root, CSRC, unit), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        return open(out).read()


def functions(text):
    """{symbol: normalised lines from its label to its .Lfunc_end} (the instruction stream and, for a kernel, its
    .amdhsa_kernel block), {kernel symbol: metadata fields}"""
    body, name, funcs = None, None, {}
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if body is None and m and not m.group(1).startswith("__hip_cuid"):
            name, body = m.group(1), []
        elif body is not None and re.match(r"^\.Lfunc_end\d+:", line):
            funcs[name], body = body, None
        elif body is not None:
            line = re.sub(r"(\.L[A-Za-z_]+)\d+_(\d+)", r"\1_\2", line.split(";")[0].rstrip())    # (comments name the index too)
            if line:
                body.append(line)
    meta = {}
    for block in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", block))
        if "name" in f:
            meta[f["name"]] = tuple(f.get(k, "0") for k in META)
    return funcs, meta


def compare(other, unit):
    (fa, ma), (fb, mb) = functions(assembly(other, unit)), functions(assembly(ROOT, unit))
    out = [f"  only in {w}: {s}" for w, x, y in (("OTHER", fa, fb), ("this tree", fb, fa)) for s in sorted(set(x) - set(y))]
    for s in sorted(set(fa) & set(fb)):
        if fa[s] != fb[s]:
            d = list(difflib.unified_diff(fa[s], fb[s], "OTHER", "this tree", lineterm="", n=1))
            out.append(f"  code differs: {s}\n" + "\n".join("    " + l for l in d[:24]))
        if ma.get(s) != mb.get(s):
            out.append(f"  metadata differs: {s}\n    {dict(zip(META, ma.get(s, ())))}\n    {dict(zip(META, mb.get(s, ())))}")
    return unit, len(fb), len(mb), out


if __name__ == "__main__":
    other = os.path.abspath(sys.argv[1])
    units = sys.argv[2:] or sorted(f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip"))
    bad = 0
    with ThreadPoolExecutor(max_workers=4) as ex:
        for unit, nf, nk, out in ex.map(lambda u: compare(other, os.path.basename(u)), units):
            print(f"{unit}: {nf} functions ({nk} kernels) " + ("identical" if not out else "DIFFER"))
            print("\n".join(out), end="\n" if out else "")
            bad += len(out)
    sys.exit(1 if bad else 0)
