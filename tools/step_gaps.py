#!/usr/bin/env python3
"""Where a Point step's time goes OUTSIDE its three streaming passes, from a rocprofv3 kernel trace.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 bench.py --no-extras --cpu-sample 0 \
      --workload C2 --steps 20 --warmup 5
  python tools/step_gaps.py DIR/**/t_kernel_trace.csv --steps 20 [--md]

A step is one `ingest -> finalize` of bench.py; the blocking finalize ends in a stream synchronise, so every step starts
on an empty queue.  The last --steps dispatches of k_bin_count are the timed steps.  Between the k_tile_accum of one step
and the k_bin_count of the next, the step boundary is the LARGEST idle gap (the host wakes up, returns to Python and
enters the next ingest there); what lies before it is the earlier step's tail, what lies after it the later step's head.
Per step:
  head   = start of k_bin_count - end of the previous step's last dispatch (host entry + whatever runs ahead of the count pass)
  ahead  = the part of head from the start of the step's first dispatch on (0 when k_bin_count is the first)
  inside = (end of k_tile_accum - start of k_bin_count) - the three passes' own durations
  tail   = end of the step's last dispatch - end of k_tile_accum
and the ordered list of dispatches.  Times in microseconds; median, min and max over the steps."""
import argparse
import collections
import csv
import re
import statistics


def short(name):
    m = re.search(r"(k_[a-z_0-9]+)", name)
    if m:
        return m.group(1)
    m = re.search(r"(fillBuffer\w*|copyBuffer\w*)", name)
    return m.group(1) if m else name.split("(")[0][-40:]


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    return rows


def steps_of(rows, nsteps):
    counts = [i for i, r in enumerate(rows) if r[2] == "k_bin_count"]
    if len(counts) < nsteps + 1:
        raise SystemExit(f"only {len(counts)} k_bin_count dispatches in the trace, need {nsteps + 1}")
    counts = counts[-(nsteps + 1):]                   # one more: the step before the first timed one closes its head

    def accum_after(i):
        for j in range(i, len(rows)):
            if rows[j][2] == "k_tile_accum":
                return j
        raise SystemExit("k_bin_count without a k_tile_accum after it")

    def boundary(acc, nxt):                           # first dispatch of the next step, between acc and its k_bin_count
        best, cut = -1, nxt
        for j in range(acc + 1, nxt + 1):
            gap = rows[j][0] - rows[j - 1][1]
            if gap > best:
                best, cut = gap, j
        return cut

    out = []
    prev_first = None
    for k, ci in enumerate(counts):
        acc = accum_after(ci)
        nxt = counts[k + 1] if k + 1 < len(counts) else None
        if nxt is None:
            last = acc
            while last + 1 < len(rows) and rows[last + 1][0] - rows[last][1] < 20_000:   # what trails the last step closely
                last += 1
            first_next = last + 1
        else:
            first_next = boundary(acc, nxt)
            last = first_next - 1
        if prev_first is not None:
            first = prev_first
            names, seen = [], collections.Counter()
            for r in rows[first:last + 1]:           # a name launched twice in a step: name, name#2
                seen[r[2]] += 1
                names.append(r[2] if seen[r[2]] == 1 else f"{r[2]}#{seen[r[2]]}")
            passes = sum(r[1] - r[0] for r in rows[ci:acc + 1] if r[2] in ("k_bin_count", "k_bin_scatter", "k_tile_accum"))
            out.append({
                "names": names,
                "head": (rows[ci][0] - rows[first - 1][1]) / 1e3,
                "ahead": (rows[ci][0] - rows[first][0]) / 1e3,
                "inside": ((rows[acc][1] - rows[ci][0]) - passes) / 1e3,
                "tail": (rows[last][1] - rows[acc][1]) / 1e3,
                "span": (rows[last][1] - rows[first - 1][1]) / 1e3,
                "dur": {n: (r[1] - r[0]) / 1e3 for n, r in zip(names, rows[first:last + 1])},
            })
        prev_first = first_next
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--md", action="store_true", help="markdown table rows")
    a = ap.parse_args()
    st = steps_of(load(a.trace), a.steps)
    lists = collections.Counter(" ".join(s["names"]) for s in st)
    print(f"{len(st)} steps; launch lists:")
    for names, c in lists.most_common():
        print(f"  {c:3d} x  {names}")

    def row(label, vals):
        med, lo, hi = statistics.median(vals), min(vals), max(vals)
        return f"| {label} | {med:.1f} | {lo:.1f} | {hi:.1f} |" if a.md else f"  {label:28s} median {med:8.1f}   min {lo:8.1f}   max {hi:8.1f}"

    if a.md:
        print("| per step, us | median | min | max |\n|---|---|---|---|")
    for key in ("head", "ahead", "inside", "tail", "span"):
        print(row(key if key != "span" else "end of previous step -> end of step", [s[key] for s in st]))
    kernels = []
    for s in st:
        for n in s["dur"]:
            if n not in kernels:
                kernels.append(n)
    for n in kernels:
        vals = [s["dur"][n] for s in st if n in s["dur"]]
        print(row(f"{n} ({len(vals)} of {len(st)} steps)", vals))


if __name__ == "__main__":
    main()
