#!/usr/bin/env python3
"""What the zonal tables cost (profiles/zonal.md).  Prints one JSON line.

One G x G grid in HBM (default 4096): the canopy band of tools/trees_time.py, its tree_id band (pcr_hip_trees), and a generated
state under it -- per cell with data a Poisson(4) number of returns at heights uniform below the canopy, folded on the host into
one cell-stats entry (N, S1, S2 at a 1 cm step) and one 64-bin histogram over [0, 32) m.  Every table the kernels make is first
compared bit for bit with the host twins.  Then each kernel is timed next to pcr_hip_copy_kernel (non-temporal) moving the same
number of bytes (a copy of B bytes reads B and writes B: the copy runs over half the bytes the kernel reads): both in one process,
alternating, each call between two device events, W warm-ups, then the MEDIAN, minimum and maximum of K timed calls.  The folds
are timed with combine = 1 (runs of equal zones summed in the wave first) and combine = 0 (one set of atomics per cell).  Last,
the whole route of Pipeline::zonal -- zone_max, a synchronise for Z, the zeroed tables, both folds, the rows, the table copied
out -- by the wall clock, against the route it replaces: the planes, the cube and the band copied to page-locked host memory.

    python tools/zonal_time.py [--grid 4096] [--steps 10] [--warmup 2] [--md profiles/zonal.md]

--md: also writes the table as Markdown."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from pcr import _cabi as A  # noqa: E402
from trees_time import band  # noqa: E402

BINS, LO, HI, RES = 64, 0.0, 32.0, 0.01
QS = [0.5, 0.95]


def state(z, seed=2):
    """(N, S1, S2, cube) of a Poisson(4) number of returns per cell with data, heights uniform in [0, canopy]."""
    rng = np.random.default_rng(seed)
    G = z.shape[0]
    top = np.where(np.isnan(z), 0.0, np.maximum(z, 0.0)).astype(np.float32).reshape(-1)
    want = rng.poisson(4.0, G * G).astype(np.uint32)
    want[np.isnan(z).reshape(-1)] = 0
    n = np.zeros(G * G, np.uint32)
    s1, s2 = np.zeros(G * G, np.int64), np.zeros(G * G, np.uint64)
    cube = np.zeros((BINS, G * G), np.uint32)
    inv_w = BINS / (HI - LO)
    for k in range(int(want.max())):
        idx = np.flatnonzero(want > k)                                   # (every cell at most once per round: += is safe)
        h = rng.uniform(0.0, 1.0, len(idx)).astype(np.float32) * top[idx]
        q = np.rint(h.astype(np.float64) / RES).astype(np.int64)
        b = np.clip(((h.astype(np.float64) - LO) * inv_w).astype(np.int64), 0, BINS - 1)
        n[idx] += 1
        s1[idx] += q
        s2[idx] += (q * q).astype(np.uint64)
        cube[b, idx] += 1
    return n.reshape(G, G), s1.reshape(G, G), s2.reshape(G, G), cube.reshape(BINS, G, G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    G = args.grid
    cells = G * G
    L = A.lib()
    if A.device_count() < 1:
        raise RuntimeError("no HIP device")
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        A.check(L.pcr_hip_event_create(C.byref(e)))

    def timed(fn, before=None):
        if before:
            before()
        A.check(L.pcr_hip_event_record(ev[0], None))
        fn()
        A.check(L.pcr_hip_event_record(ev[1], None))
        ms = C.c_float(0.0)
        A.check(L.pcr_hip_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        return ms.value

    # ---- the scene: canopy -> tree_id on the device, the state under it
    z = band(G)
    d_src = A.DeviceBuffer.from_numpy(z)
    d_id, d_h = A.DeviceBuffer(4 * cells), A.DeviceBuffer(4 * cells)
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_trees_work_bytes(G, G, C.byref(nbytes)))
    work = A.DeviceBuffer(nbytes.value)
    tp = A.TreeParams()
    A.check(L.pcr_hip_trees(d_src.ptr, G, G, G, C.byref(tp), d_id.ptr, G, d_h.ptr, G, work.ptr, nbytes.value, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    labels = d_id.to_numpy(np.float32, (G, G))
    for d in (d_src, d_h, work):
        d.free()
    n, s1, s2, cube = state(z)
    d_n, d_s1, d_s2, d_cube = (A.DeviceBuffer.from_numpy(a) for a in (n, s1, s2, cube))

    d_max = A.DeviceBuffer(4)
    A.check(L.pcr_hip_zone_max(d_id.ptr, G, G, G, d_max.ptr, None))
    Z = int(d_max.to_numpy(np.uint32, (1,))[0])
    hz = C.c_uint32(0)
    A.check(L.pcr_hip_zone_max_host(labels.ctypes.data, G, G, G, C.byref(hz)))
    assert Z == hz.value and Z >= 1, (Z, hz.value)

    tab = {k: A.DeviceBuffer(8 * Z) for k in ("cells", "n", "s1", "s2", "hist_n")}
    d_counts = A.DeviceBuffer(8 * Z * BINS)
    cols = {k: A.DeviceBuffer(4 * Z) for k in ("mean", "var", "std", "p0", "p1")}
    q = np.array(QS, np.float32)
    w = (HI - LO) / BINS
    pct_ptrs = (C.c_void_p * 2)(cols["p0"].ptr, cols["p1"].ptr)

    def zero_stats():
        for k in ("cells", "n", "s1", "s2"):
            A.check(L.pcr_hip_memset(tab[k].ptr, 0, 8 * Z, None))

    def zero_hist():
        A.check(L.pcr_hip_memset(d_counts.ptr, 0, 8 * Z * BINS, None))

    def zone_max():
        A.check(L.pcr_hip_zone_max(d_id.ptr, G, G, G, d_max.ptr, None))

    def fold_stats(combine=1):
        p = A.ZoneFoldParams(combine)
        A.check(L.pcr_hip_zone_fold_stats(d_id.ptr, G, G, G, d_n.ptr, d_s1.ptr, d_s2.ptr, G, Z, C.byref(p), tab["cells"].ptr, tab["n"].ptr,
                                          tab["s1"].ptr, tab["s2"].ptr, None))

    def fold_hist(combine=1):
        p = A.ZoneFoldParams(combine)
        A.check(L.pcr_hip_zone_fold_hist(d_id.ptr, G, G, G, d_cube.ptr, BINS, G, cells, Z, C.byref(p), d_counts.ptr, None))

    def rows_stats():
        A.check(L.pcr_hip_zone_rows_stats(tab["n"].ptr, tab["s1"].ptr, tab["s2"].ptr, Z, 0.0, RES, 1, cols["mean"].ptr, cols["var"].ptr,
                                          cols["std"].ptr, None))

    def rows_pct():
        A.check(L.pcr_hip_zone_rows_percentiles(d_counts.ptr, BINS, Z, LO, w, 2, q.ctypes.data, tab["hist_n"].ptr, pct_ptrs, None))

    # ---- every table against the host twins, both fold forms
    hp = A.ZoneFoldParams(1)
    want = {k: np.zeros(Z, t) for k, t in (("cells", np.uint64), ("n", np.uint64), ("s1", np.int64), ("s2", np.uint64), ("hist_n", np.uint64))}
    want_counts = np.zeros((Z, BINS), np.uint64)
    A.check(L.pcr_hip_zone_fold_stats_host(labels.ctypes.data, G, G, G, n.ctypes.data, s1.ctypes.data, s2.ctypes.data, G, Z, C.byref(hp),
                                           want["cells"].ctypes.data, want["n"].ctypes.data, want["s1"].ctypes.data, want["s2"].ctypes.data))
    A.check(L.pcr_hip_zone_fold_hist_host(labels.ctypes.data, G, G, G, cube.ctypes.data, BINS, G, cells, Z, C.byref(hp),
                                          want_counts.ctypes.data))
    want_cols = {k: np.zeros(Z, np.float32) for k in cols}
    A.check(L.pcr_hip_zone_rows_stats_host(want["n"].ctypes.data, want["s1"].ctypes.data, want["s2"].ctypes.data, Z, 0.0, RES, 1,
                                           want_cols["mean"].ctypes.data, want_cols["var"].ctypes.data, want_cols["std"].ctypes.data))
    hptrs = (C.c_void_p * 2)(want_cols["p0"].ctypes.data, want_cols["p1"].ctypes.data)
    A.check(L.pcr_hip_zone_rows_percentiles_host(want_counts.ctypes.data, BINS, Z, LO, w, 2, q.ctypes.data, want["hist_n"].ctypes.data, hptrs))
    for combine in (1, 0):
        zero_stats()
        zero_hist()
        fold_stats(combine)
        fold_hist(combine)
        rows_stats()
        rows_pct()
        for k in want:
            assert np.array_equal(tab[k].to_numpy(want[k].dtype, (Z,)), want[k]), f"{k} differs from the host twin (combine {combine})"
        assert np.array_equal(d_counts.to_numpy(np.uint64, (Z, BINS)), want_counts), f"counts differ from the host twin (combine {combine})"
        for k in cols:
            assert np.array_equal(cols[k].to_numpy(np.float32, (Z,)).view(np.uint32), want_cols[k].view(np.uint32)), f"{k} differs"
    zoned = int(want["cells"].sum())

    # ---- the kernels and the copy kernel over the same bytes, alternating
    copy_dst = A.DeviceBuffer((4 + 4 * BINS) * cells // 2 + 256)
    cases = [("k_zone_max", zone_max, None, 4 * cells),
             ("k_zone_fold_stats, combine 1", lambda: fold_stats(1), zero_stats, 24 * cells),
             ("k_zone_fold_stats, combine 0", lambda: fold_stats(0), zero_stats, 24 * cells),
             ("k_zone_fold_hist, combine 1", lambda: fold_hist(1), zero_hist, (4 + 4 * BINS) * cells),
             ("k_zone_fold_hist, combine 0", lambda: fold_hist(0), zero_hist, (4 + 4 * BINS) * cells),
             ("k_zone_rows_stats", rows_stats, None, 24 * Z),
             ("k_zone_rows_pct", rows_pct, None, 8 * BINS * Z)]
    times = {name: ([], []) for name, _, _, _ in cases}
    for i in range(args.warmup + args.steps):
        for name, fn, before, read in cases:
            half = max(read // 2 // 16 * 16, 16)
            a = timed(fn, before)
            b = timed(lambda: A.check(L.pcr_hip_copy_kernel(copy_dst.ptr, d_cube.ptr, half, 1, None)))
            if i >= args.warmup:
                times[name][0].append(a)
                times[name][1].append(b)
    A.check(L.pcr_hip_stream_synchronize(None))
    rows = []
    for name, _, _, read in cases:
        a, b = times[name]
        ma, mb = statistics.median(a), statistics.median(b)
        rows.append({"kernel": name, "ms": round(ma, 4), "ms_min_max": [round(min(a), 4), round(max(a), 4)], "bytes_read": read,
                     "copy_ms": round(mb, 4), "copy_ms_min_max": [round(min(b), 4), round(max(b), 4)], "ratio_to_copy": round(ma / mb, 2)})

    # ---- the whole route of Pipeline::zonal by the wall clock, against the copy-out it replaces
    out = {k: np.zeros(Z, t) for k, t in (("cells", np.uint64), ("n", np.uint64), ("hist_n", np.uint64))}
    out_cols = {k: np.zeros(Z, np.float32) for k in cols}
    host_max = np.zeros(1, np.uint32)

    def whole():
        t0 = time.perf_counter()
        zone_max()
        A.check(L.pcr_hip_memcpy_d2h(host_max.ctypes.data, d_max.ptr, 4, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        zero_stats()
        zero_hist()
        fold_stats(1)
        rows_stats()
        fold_hist(1)
        rows_pct()
        for k in out:
            A.check(L.pcr_hip_memcpy_d2h(out[k].ctypes.data, tab[k].ptr, 8 * Z, None))
        for k in out_cols:
            A.check(L.pcr_hip_memcpy_d2h(out_cols[k].ctypes.data, cols[k].ptr, 4 * Z, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        return (time.perf_counter() - t0) * 1e3

    pinned = C.c_void_p()
    route_bytes = (4 + 20 + 4 * BINS) * cells
    A.check(L.pcr_hip_host_alloc(C.byref(pinned), route_bytes))

    def copy_out():
        t0 = time.perf_counter()
        at = pinned.value
        for d, size in ((d_id, 4 * cells), (d_n, 4 * cells), (d_s1, 8 * cells), (d_s2, 8 * cells), (d_cube, 4 * BINS * cells)):
            A.check(L.pcr_hip_memcpy_d2h(at, d.ptr, size, None))
            at += size
        A.check(L.pcr_hip_stream_synchronize(None))
        return (time.perf_counter() - t0) * 1e3

    t_whole, t_out = [], []
    for i in range(args.warmup + args.steps):
        a, b = whole(), copy_out()
        if i >= args.warmup:
            t_whole.append(a)
            t_out.append(b)
    A.check(L.pcr_hip_host_free(pinned))
    total = {"grid": G, "zones": Z, "cells_in_a_zone": zoned, "bins": BINS, "steps": args.steps, "warmup": args.warmup,
             "equals_host_twins": True, "kernels": rows, "whole_call_ms": round(statistics.median(t_whole), 3),
             "whole_call_ms_min_max": [round(min(t_whole), 3), round(max(t_whole), 3)], "copy_out_ms": round(statistics.median(t_out), 3),
             "copy_out_ms_min_max": [round(min(t_out), 3), round(max(t_out), 3)], "copy_out_bytes": route_bytes,
             "table_bytes": Z * (3 * 8 + 5 * 4)}
    print(json.dumps(total), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"Zonal tables on a {G} x {G} grid: the tree_id band of the generated canopy ({Z} zones, {zoned} cells in one), one "
                    f"cell-stats entry and one {BINS}-bin histogram; every table equal to the host twins bit for bit, with combine = 1 and "
                    f"combine = 0.  Median of {args.steps} after {args.warmup} warm-ups (min .. max), each kernel alternating with the "
                    f"non-temporal copy kernel moving the bytes the kernel reads.\n\n")
            f.write("| kernel | ms | bytes read | copy of the same bytes, ms | kernel / copy |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['kernel']} | {r['ms']:.3f} ({r['ms_min_max'][0]:.3f} .. {r['ms_min_max'][1]:.3f}) | {r['bytes_read']} | "
                        f"{r['copy_ms']:.3f} ({r['copy_ms_min_max'][0]:.3f} .. {r['copy_ms_min_max'][1]:.3f}) | {r['ratio_to_copy']:.2f} |\n")
            f.write(f"\nThe whole route of Pipeline::zonal by the wall clock (zone_max, the synchronise for Z, zeroed tables, both folds, "
                    f"the rows, {total['table_bytes']} bytes of table copied out): {total['whole_call_ms']:.2f} ms "
                    f"({min(t_whole):.2f} .. {max(t_whole):.2f}).  The route it replaces, the band, the planes and the cube "
                    f"({route_bytes} bytes) copied to page-locked host memory, before any grouping on the host: "
                    f"{total['copy_out_ms']:.1f} ms ({min(t_out):.1f} .. {max(t_out):.1f}).\n")


if __name__ == "__main__":
    main()
