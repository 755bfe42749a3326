#!/usr/bin/env python3
"""What pcr_hip_trees costs (profiles/trees.md).  Prints one JSON line per case.

One G x G float32 canopy band in HBM (default 4096): Gaussian crowns of height 3..30 m and sigma 1..4 cells, about one per 60
cells, combined by maximum, noise, values rounded to 0.25, 5 % NaN cells.  The whole device result -- both bands and every
column of the table -- is first compared bit for bit with the host twin.  Then pcr_hip_trees is timed next to
pcr_hip_copy_kernel (non-temporal) on the same band: both in one process, alternating, each call between two device events, W
warm-ups, then the MEDIAN, minimum and maximum of K timed calls.  The phases are timed by difference: stop_after = 1..4 enqueues
only the first phases (cells, discs, numbering, jumping), the whole call adds the labels.  The copy kernel moves two bands (one
read, one written); `bands_moved` counts what a phase reads and writes in band-sized (4 bytes per cell) units, and
`per_band_ratio` is the phase's time over the copy kernel's scaled to the same bytes.

    python tools/trees_time.py [--grid 4096] [--steps 10] [--warmup 2] [--md profiles/trees.md]

--md: also writes the table as Markdown."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))

import numpy as np  # noqa: E402

from pcr import _cabi as A  # noqa: E402

PHASES = ["cells (3 x 3)", "discs", "numbering", "jumping", "labels"]
# band-sized arrays a phase reads + writes: cells src -> root, top, count; discs root (+ a few discs of src) -> a few words;
# numbering top twice -> top; a jumping ROUND THAT WORKS root + the gathered root -> part of root (counted per such round);
# labels root, the gathered top and src -> two bands (+ the atomics)
MOVED = [4.0, 1.0, 3.0, 2.0, 5.0]


def band(G):
    rng = np.random.default_rng(1)
    z = np.zeros((G, G), np.float32)
    n = G * G // 60
    r0, c0 = rng.uniform(0, G, n), rng.uniform(0, G, n)
    a, s = rng.uniform(3.0, 30.0, n).astype(np.float32), rng.uniform(1.0, 4.0, n)
    for k in range(n):                                               # (each crown touches its own 4-sigma box only)
        R = int(4 * s[k]) + 1
        ra, rb, ca, cb = max(0, int(r0[k]) - R), min(G, int(r0[k]) + R + 1), max(0, int(c0[k]) - R), min(G, int(c0[k]) + R + 1)
        rr, cc = np.mgrid[ra:rb, ca:cb]
        bump = a[k] * np.exp(-((rr - r0[k]) ** 2 + (cc - c0[k]) ** 2) / (2.0 * s[k] * s[k]))
        z[ra:rb, ca:cb] = np.maximum(z[ra:rb, ca:cb], bump.astype(np.float32))
    z = z + rng.normal(0.0, 0.3, (G, G)).astype(np.float32)
    z = (np.round(z * 4.0) / 4.0).astype(np.float32)
    z[rng.uniform(size=(G, G)) < 0.05] = np.nan
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    G = args.grid
    L = A.lib()
    if A.device_count() < 1:
        raise RuntimeError("no HIP device")
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        A.check(L.pcr_hip_event_create(C.byref(e)))

    def timed(fn):
        A.check(L.pcr_hip_event_record(ev[0], None))
        fn()
        A.check(L.pcr_hip_event_record(ev[1], None))
        ms = C.c_float(0.0)
        A.check(L.pcr_hip_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        return ms.value

    z = band(G)
    src = A.DeviceBuffer.from_numpy(z)
    d_id, d_h, copy_dst = (A.DeviceBuffer(4 * G * G) for _ in range(3))
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_trees_work_bytes(G, G, C.byref(nbytes)))
    work = A.DeviceBuffer(nbytes.value)

    def run(stop_after=0):
        p = A.TreeParams(stop_after=stop_after)
        A.check(L.pcr_hip_trees(src.ptr, G, G, G, C.byref(p), d_id.ptr, G, d_h.ptr, G, work.ptr, nbytes.value, None))

    def copy():
        A.check(L.pcr_hip_copy_kernel(copy_dst.ptr, src.ptr, 4 * G * G, 1, None))

    # ---- the whole result against the host twin
    run()
    n, rounds = C.c_int64(0), C.c_int(0)
    A.check(L.pcr_hip_trees_count(work.ptr, nbytes.value, C.byref(n), C.byref(rounds), None))
    T = n.value
    cols = [A.DeviceBuffer(max(T, 1) * 4) for _ in range(4)]
    A.check(L.pcr_hip_trees_table(src.ptr, G, G, G, work.ptr, nbytes.value, T, *[c.ptr for c in cols], None))
    A.check(L.pcr_hip_stream_synchronize(None))
    want_id, want_h = np.empty((G, G), np.float32), np.empty((G, G), np.float32)
    want = [np.empty(max(T, 1), t) for t in (np.int32, np.int32, np.float32, np.int32)]
    hn = C.c_int64(0)
    hp = A.TreeParams()
    A.check(L.pcr_hip_trees_host(z.ctypes.data, G, G, G, C.byref(hp), want_id.ctypes.data, G, want_h.ctypes.data, G, C.byref(hn), T,
                                 *[w.ctypes.data for w in want]))
    assert hn.value == T, f"{T} trees on the device, {hn.value} on the host"
    assert np.array_equal(d_id.to_numpy(np.float32, (G, G)).view(np.uint32), want_id.view(np.uint32)), "tree_id differs from the host twin"
    assert np.array_equal(d_h.to_numpy(np.float32, (G, G)).view(np.uint32), want_h.view(np.uint32)), "tree_height differs from the host twin"
    for c, w, name in zip(cols, want, ("row", "col", "height", "crown_cells")):
        assert np.array_equal(c.to_numpy(w.dtype, w.shape)[:T].view(np.uint32), w[:T].view(np.uint32)), f"table.{name} differs from the host twin"
    labelled = int((~np.isnan(want_id)).sum())

    # ---- timing: the prefixes and the copy kernel, alternating
    t = {k: [] for k in (1, 2, 3, 4, 0)}
    t_copy = []
    for i in range(args.warmup + args.steps):
        for k in t:
            a, b = timed(lambda: run(k)), timed(copy)
            if i >= args.warmup:
                t[k].append(a)
                t_copy.append(b)
    A.check(L.pcr_hip_stream_synchronize(None))
    med = {k: statistics.median(v) for k, v in t.items()}
    mc = statistics.median(t_copy)
    prefix = [med[1], med[2], med[3], med[4], med[0]]
    rows = []
    for j, name in enumerate(PHASES):
        ms = prefix[j] - (prefix[j - 1] if j else 0.0)
        moved = MOVED[j] * (max(rounds.value, 1) if name == "jumping" else 1)
        rows.append({"phase": name, "ms": round(ms, 4), "bands_moved": moved, "per_band_ratio": round(ms / (mc * moved / 2.0), 2)})
    total = {"grid": G, "trees": T, "labelled_cells": labelled, "rounds_enqueued": int(np.ceil(np.log2(G * G))) + 1,
             "rounds_that_worked": rounds.value, "steps": args.steps, "warmup": args.warmup, "kernel_ms": round(med[0], 4),
             "kernel_ms_min_max": [round(min(t[0]), 4), round(max(t[0]), 4)], "copy_kernel_ms": round(mc, 4),
             "copy_kernel_ms_min_max": [round(min(t_copy), 4), round(max(t_copy), 4)], "work_bytes_per_cell": round(nbytes.value / (G * G), 2),
             "equals_host_twin": True, "phases": rows}
    print(json.dumps(total), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"pcr_hip_trees on a {G} x {G} canopy band: {T} trees, {labelled} labelled cells, the whole result equal to the host "
                    f"twin bit for bit.  {total['rounds_enqueued']} jumping rounds enqueued, {rounds.value} changed a pointer.  Whole "
                    f"call {med[0]:.3f} ms (min {min(t[0]):.3f}, max {max(t[0]):.3f}; median of {args.steps} after {args.warmup} "
                    f"warm-ups); copy kernel on the same band {mc:.3f} ms ({min(t_copy):.3f} .. {max(t_copy):.3f}).  Work area: "
                    f"{total['work_bytes_per_cell']} bytes per cell.  Phases by difference of stop_after prefixes.\n\n")
            f.write("| phase | ms | bands moved | phase / copy per band moved |\n|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['phase']} | {r['ms']:.3f} | {r['bands_moved']:g} | {r['per_band_ratio']:.2f} |\n")


if __name__ == "__main__":
    main()
