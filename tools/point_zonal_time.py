#!/usr/bin/env python3
"""What the point zonal tables cost (profiles/point_zonal.md).  Prints one JSON line.

N points (default 50 M) over the 4096 x 4096 canopy of tools/trees_time.py, about three per cell in row-major order of their
cells: a height below the canopy as the value, a mask that keeps every point, and three labellings -- 100 square plots, 2 025
square stands, and the tree_id band (pcr_hip_trees) sampled at the point's cell -- each in the generated, spatially coherent order
and in a shuffled one.  Per case the stats fold and a 64-bin histogram fold run with path 1 (global atomics) and, where the table
fits, path 2 (a workgroup-private LDS table); the first million points' tables are first compared bit for bit with the host twins.
Each kernel is timed next to pcr_hip_copy_kernel (non-temporal) moving the bytes the kernel reads (a copy of B bytes reads B and
writes B: the copy runs over half of them): both in one process, alternating, each call between two device events, W warm-ups,
then the MEDIAN, minimum and maximum of K timed calls.  Then, on the coherent and the shuffled plots: the workgroups per CU
(`blocks`) swept for both paths, and path 2 with the table's capacity raised to 1 024 and to the greatest it takes (the LDS a
workgroup asks for, hence the workgroups a CU holds).  Last, the whole route of Pipeline::point_zonal by the wall clock -- both
folds, the info words, the rows, the table copied out -- against the route it replaces: label and value copied to page-locked
host memory.

    python tools/point_zonal_time.py [--points 50000000] [--steps 10] [--warmup 2] [--md profiles/point_zonal.md]
"""
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

G = 4096
BINS, LO, HI, RES = 64, 0.0, 64.0, 0.01
QS = [0.5, 0.95]
CHECK = 1 << 20                              # points whose tables are compared with the twins'


def tree_ids(L, z):
    d_src = A.DeviceBuffer.from_numpy(z)
    d_id, d_h = A.DeviceBuffer(4 * G * G), A.DeviceBuffer(4 * G * G)
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_trees_work_bytes(G, G, C.byref(nbytes)))
    work = A.DeviceBuffer(nbytes.value)
    tp = A.TreeParams()
    A.check(L.pcr_hip_trees(d_src.ptr, G, G, G, C.byref(tp), d_id.ptr, G, d_h.ptr, G, work.ptr, nbytes.value, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    ids = d_id.to_numpy(np.float32, (G, G))
    for d in (d_src, d_id, d_h, work):
        d.free()
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    n = args.points
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

    # ---- the scene
    z = band(G)
    ids = tree_ids(L, z)
    rng = np.random.default_rng(5)
    cell = (np.arange(n, dtype=np.int64) * (G * G) // n)
    r, c = cell // G, cell % G
    top = np.where(np.isnan(z), 0.0, np.maximum(z, 0.0)).astype(np.float32).reshape(-1)
    value = rng.random(n, dtype=np.float32) * top[cell]
    labellings = {"100 plots": ((r // 410) * 10 + c // 410 + 1).astype(np.float32),
                  "2 025 stands": ((r // 92) * 45 + c // 92 + 1).astype(np.float32),
                  "trees": ids.reshape(-1)[cell]}
    del r, c, cell, top
    perm = rng.permutation(n)
    mask = np.ones(n, np.uint8)
    d_mask = A.DeviceBuffer.from_numpy(mask)
    d_copy_dst, d_copy_src = A.DeviceBuffer(9 * n // 2 + 256), A.DeviceBuffer(9 * n // 2 + 256)
    A.check(L.pcr_hip_memset(d_copy_src.ptr, 0, 9 * n // 2 + 256, None))
    d_value = {"coherent": A.DeviceBuffer.from_numpy(value), "shuffled": A.DeviceBuffer.from_numpy(value[perm])}
    h_value = {"coherent": value, "shuffled": value[perm]}
    inv_res, inv_w, w = 1.0 / RES, BINS / (HI - LO), (HI - LO) / BINS
    cap_s = A.POINT_FOLD_LDS_BYTES // A.POINT_FOLD_STATS_ROW_BYTES
    cap_h = A.POINT_FOLD_LDS_BYTES // (4 * BINS)

    rows, checked = [], 0
    sweeps = []
    whole = {}
    for lname, lab in labellings.items():
        Z = int(np.nanmax(lab))
        for order in ("coherent", "shuffled"):
            h_lab = lab if order == "coherent" else lab[perm]
            d_lab = A.DeviceBuffer.from_numpy(h_lab)
            dv = d_value[order]
            t_pts, t_n, t_s1, t_s2 = (A.DeviceBuffer(8 * Z) for _ in range(4))
            t_info = A.DeviceBuffer(16)
            t_counts = A.DeviceBuffer(8 * Z * BINS)

            def zero_stats():
                for t in (t_pts, t_n, t_s1, t_s2):
                    A.check(L.pcr_hip_memset(t.ptr, 0, 8 * Z, None))
                A.check(L.pcr_hip_memset(t_info.ptr, 0, 16, None))

            def zero_hist():
                A.check(L.pcr_hip_memset(t_counts.ptr, 0, 8 * Z * BINS, None))

            def fold_stats(path, blocks=0, count=n, cap=None):
                p = A.PointFoldParams(path, blocks)
                A.check(L.pcr_hip_point_fold_stats(d_lab.ptr, d_mask.ptr, dv.ptr, count, 0.0, inv_res, cap or Z, C.byref(p), t_pts.ptr, t_n.ptr,
                                                   t_s1.ptr, t_s2.ptr, t_info.ptr, None))

            def fold_hist(path, blocks=0, count=n):
                p = A.PointFoldParams(path, blocks)
                A.check(L.pcr_hip_point_fold_hist(d_lab.ptr, d_mask.ptr, dv.ptr, count, BINS, LO, inv_w, Z, C.byref(p), t_counts.ptr, None, None))

            # the first million points against the twins
            m = min(CHECK, n)
            want = {k: np.zeros(Z, t) for k, t in (("pts", np.uint64), ("n", np.uint64), ("s1", np.int64), ("s2", np.uint64))}
            want_info, want_counts = np.zeros(2, np.uint64), np.zeros((Z, BINS), np.uint64)
            hp = A.PointFoldParams(0, 0)
            hv = h_value[order]
            A.check(L.pcr_hip_point_fold_stats_host(h_lab.ctypes.data, mask.ctypes.data, hv.ctypes.data, m, 0.0, inv_res, Z, C.byref(hp),
                                                    want["pts"].ctypes.data, want["n"].ctypes.data, want["s1"].ctypes.data,
                                                    want["s2"].ctypes.data, want_info.ctypes.data))
            A.check(L.pcr_hip_point_fold_hist_host(h_lab.ctypes.data, mask.ctypes.data, hv.ctypes.data, m, BINS, LO, inv_w, Z, C.byref(hp),
                                                   want_counts.ctypes.data, None))
            paths_s = [1] + ([2] if Z <= cap_s else [])
            paths_h = [1] + ([2] if Z <= cap_h else [])
            for path in paths_s:
                zero_stats()
                fold_stats(path, count=m)
                for k, t in (("pts", t_pts), ("n", t_n), ("s1", t_s1), ("s2", t_s2)):
                    assert np.array_equal(t.to_numpy(want[k].dtype, (Z,)), want[k]), f"{lname} {order} path {path}: {k} differs from the twin"
                assert np.array_equal(t_info.to_numpy(np.uint64, (2,)), want_info), "info differs from the twin"
            for path in paths_h:
                zero_hist()
                fold_hist(path, count=m)
                assert np.array_equal(t_counts.to_numpy(np.uint64, (Z, BINS)), want_counts), f"{lname} {order} path {path}: counts differ"
            checked += 1

            def run(cases):
                times = {name: ([], []) for name, _, _ in cases}
                half = 9 * n // 2 // 16 * 16
                for i in range(args.warmup + args.steps):
                    for name, fn, before in cases:
                        a = timed(fn, before)
                        b = timed(lambda: A.check(L.pcr_hip_copy_kernel(d_copy_dst.ptr, d_copy_src.ptr, half, 1, None)))
                        if i >= args.warmup:
                            times[name][0].append(a)
                            times[name][1].append(b)
                A.check(L.pcr_hip_stream_synchronize(None))
                out = []
                for name, _, _ in cases:
                    a, b = times[name]
                    ma, mb = statistics.median(a), statistics.median(b)
                    out.append({"case": name, "ms": round(ma, 4), "ms_min_max": [round(min(a), 4), round(max(a), 4)], "copy_ms": round(mb, 4),
                                "ratio_to_copy": round(ma / mb, 2)})
                return out

            cases = [(f"stats, path {p}", (lambda p=p: fold_stats(p)), zero_stats) for p in paths_s] + \
                    [(f"hist, path {p}", (lambda p=p: fold_hist(p)), zero_hist) for p in paths_h]
            for row in run(cases):
                row.update(labels=lname, zones=Z, order=order)
                rows.append(row)

            if lname == "100 plots":
                sw = [(f"stats, path {p}, {b} workgroups per CU", (lambda p=p, b=b: fold_stats(p, 256 * b)), zero_stats)
                      for p in (1, 2) for b in (1, 2, 4, 8, 16)]
                sw += [(f"hist, path {p}, {b} workgroups per CU", (lambda p=p, b=b: fold_hist(p, 256 * b)), zero_hist)
                       for p in (1, 2) for b in (2, 4, 8)]
                for row in run(sw):
                    row.update(order=order)
                    sweeps.append(row)
                # the same labels in a table of greater capacity: more LDS per workgroup, fewer workgroups per CU
                big = A.DeviceBuffer(8 * cap_s * 4)
                keep = (t_pts, t_n, t_s1, t_s2)
                t_pts, t_n, t_s1, t_s2 = (C.c_void_p(big.ptr.value + 8 * cap_s * k) for k in range(4))

                class P:                                                 # (a pointer with .ptr, like a DeviceBuffer)
                    def __init__(self, v):
                        self.ptr = v
                t_pts, t_n, t_s1, t_s2 = (P(v) for v in (t_pts, t_n, t_s1, t_s2))

                def zero_big():
                    A.check(L.pcr_hip_memset(big.ptr, 0, 8 * cap_s * 4, None))
                    A.check(L.pcr_hip_memset(t_info.ptr, 0, 16, None))
                cs_ = [(f"stats, path 2, capacity {cap} ({cap * A.POINT_FOLD_STATS_ROW_BYTES} B of LDS)", (lambda cap=cap: fold_stats(2, cap=cap)),
                        zero_big) for cap in (100, 1024, cap_s)]
                for row in run(cs_):
                    row.update(order=order)
                    sweeps.append(row)
                t_pts, t_n, t_s1, t_s2 = keep
                big.free()

            if order == "coherent" and lname != "2 025 stands":
                # the whole route by the wall clock against the copy-out it replaces
                cols = [A.DeviceBuffer(4 * Z) for _ in range(5)]
                t_hn = A.DeviceBuffer(8 * Z)
                q = np.array(QS, np.float32)
                ptrs = (C.c_void_p * 2)(cols[3].ptr, cols[4].ptr)
                info = np.zeros(2, np.uint64)
                outs = [np.zeros(Z, np.uint64) for _ in range(3)] + [np.zeros(Z, np.float32) for _ in range(5)]

                def route(table_only):
                    if not table_only:
                        zero_stats()
                        zero_hist()
                        A.check(L.pcr_hip_stream_synchronize(None))
                    t0 = time.perf_counter()
                    if not table_only:
                        fold_stats(0)
                        fold_hist(0)
                    A.check(L.pcr_hip_memcpy_d2h(info.ctypes.data, t_info.ptr, 16, None))
                    A.check(L.pcr_hip_stream_synchronize(None))
                    top_ = int(info[0])
                    A.check(L.pcr_hip_zone_rows_stats(t_n.ptr, t_s1.ptr, t_s2.ptr, top_, 0.0, RES, 1, cols[0].ptr, cols[1].ptr, cols[2].ptr, None))
                    A.check(L.pcr_hip_zone_rows_percentiles(t_counts.ptr, BINS, top_, LO, w, 2, q.ctypes.data, t_hn.ptr, ptrs, None))
                    for o, d in zip(outs, (t_pts, t_n, t_hn) + tuple(cols)):
                        A.check(L.pcr_hip_memcpy_d2h(o.ctypes.data, d.ptr, o.nbytes, None))
                    A.check(L.pcr_hip_stream_synchronize(None))
                    return (time.perf_counter() - t0) * 1e3

                pinned = C.c_void_p()
                A.check(L.pcr_hip_host_alloc(C.byref(pinned), 8 * n))

                def copy_out():
                    t0 = time.perf_counter()
                    A.check(L.pcr_hip_memcpy_d2h(pinned.value, d_lab.ptr, 4 * n, None))
                    A.check(L.pcr_hip_memcpy_d2h(pinned.value + 4 * n, dv.ptr, 4 * n, None))
                    A.check(L.pcr_hip_stream_synchronize(None))
                    return (time.perf_counter() - t0) * 1e3

                t_a, t_b, t_c = [], [], []
                for i in range(args.warmup + args.steps):
                    a, b, c_ = route(False), route(True), copy_out()
                    if i >= args.warmup:
                        t_a.append(a)
                        t_b.append(b)
                        t_c.append(c_)
                A.check(L.pcr_hip_host_free(pinned))
                whole[lname] = {"zones": Z, "folds_and_table_ms": round(statistics.median(t_a), 3),
                                "folds_and_table_min_max": [round(min(t_a), 3), round(max(t_a), 3)],
                                "table_alone_ms": round(statistics.median(t_b), 3), "table_alone_min_max": [round(min(t_b), 3), round(max(t_b), 3)],
                                "copy_out_ms": round(statistics.median(t_c), 3), "copy_out_min_max": [round(min(t_c), 3), round(max(t_c), 3)],
                                "copy_out_bytes": 8 * n, "table_bytes": Z * (3 * 8 + 5 * 4)}
                for d in cols + [t_hn]:
                    d.free()
            for d in (d_lab, t_pts, t_n, t_s1, t_s2, t_info, t_counts):
                d.free()

    total = {"points": n, "bins": BINS, "steps": args.steps, "warmup": args.warmup, "first_million_equal_host_twins": checked,
             "bytes_read": 9 * n, "lds_bytes": A.POINT_FOLD_LDS_BYTES, "kernels": rows, "sweeps": sweeps, "whole": whole}
    print(json.dumps(total), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"Point zonal tables over {n} points ({9 * n} bytes read per fold: label, mask, value), a stats fold and a {BINS}-bin "
                    f"histogram fold; the first {min(CHECK, n)} points' tables equal to the host twins bit for bit in all {checked} cases, on "
                    f"every path timed.  Median of {args.steps} after {args.warmup} warm-ups (min .. max), each kernel alternating with "
                    f"the non-temporal copy kernel moving the bytes the kernel reads.\n\n")
            f.write("| labels | zones | order | fold | ms | copy of the same bytes, ms | kernel / copy |\n|---|---|---|---|---|---|---|\n")
            for r_ in rows:
                f.write(f"| {r_['labels']} | {r_['zones']} | {r_['order']} | {r_['case']} | {r_['ms']:.3f} ({r_['ms_min_max'][0]:.3f} .. "
                        f"{r_['ms_min_max'][1]:.3f}) | {r_['copy_ms']:.3f} | {r_['ratio_to_copy']:.2f} |\n")
            f.write("\nThe 100 plots again: workgroups per CU (of 256 CUs), and path 2 with a table of greater capacity.\n\n")
            f.write("| order | case | ms | kernel / copy |\n|---|---|---|---|\n")
            for r_ in sweeps:
                f.write(f"| {r_['order']} | {r_['case']} | {r_['ms']:.3f} ({r_['ms_min_max'][0]:.3f} .. {r_['ms_min_max'][1]:.3f}) | "
                        f"{r_['ratio_to_copy']:.2f} |\n")
            f.write("\nThe whole route by the wall clock, path 0: both folds, the info words, the rows and the table copied out; the table "
                    "alone (what Pipeline::point_zonal does after the ingests); and the route it replaces, label and value copied to "
                    "page-locked host memory before any grouping there.\n\n")
            f.write("| labels | zones | folds and table, ms | table alone, ms | copy-out, ms | copy-out bytes | table bytes |\n|---|---|---|---|---|---|---|\n")
            for k, v in whole.items():
                f.write(f"| {k} | {v['zones']} | {v['folds_and_table_ms']:.2f} ({v['folds_and_table_min_max'][0]:.2f} .. "
                        f"{v['folds_and_table_min_max'][1]:.2f}) | {v['table_alone_ms']:.2f} | {v['copy_out_ms']:.1f} "
                        f"({v['copy_out_min_max'][0]:.1f} .. {v['copy_out_min_max'][1]:.1f}) | {v['copy_out_bytes']} | {v['table_bytes']} |\n")


if __name__ == "__main__":
    main()
