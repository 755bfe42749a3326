#!/usr/bin/env python3
"""What the exact point-in-polygon test costs (profiles/points_in_polygons.md).  Prints one JSON line.

N points (default 50 M) spread uniformly over a G x G extent (default 4096), against tools/rasterize_time.py's three polygon sets:
  plots      10 000 disjoint 32-gons of about 11 units radius on a lattice
  stands     a jittered partition of the extent into about 2 000 polygons of about 200 vertices with shared edges
  one        one polygon of 100 000 vertices covering most of the extent
For each, the kernel's answer for the first million points is first compared bit for bit with the host twin's.  Then K timed calls
after W warm-ups, each pcr_hip_points_in_polygons (between the two events the call records) alternating with pcr_hip_copy_kernel
(non-temporal) copying 10 bytes per point -- 10 read and 10 written: the 20 bytes per point the kernel itself must move (x, y in,
the channel out).  Beside them:
  the cell-resolution route it complements: pcr_hip_sample_grid NEAREST on the label band pcr_hip_rasterize_polygons burns on the
  G x G unit grid (the band is made once, outside the timing);
  the index build (pcr_hip_polygon_index_create) and its upload, by the wall clock;
  the host twin on 16 threads over the first million points, scaled to N by the wall clock (said so in the table);
  the index's cols, rows, items, listed edges and bytes.

--sides times further index sizes beside the automatic one (the builder's rule is judged by these rows).

    python tools/points_in_polygons_time.py [--points 50000000] [--grid 4096] [--steps 10] [--warmup 2] [--sides 0,512,256]
                                            [--md profiles/points_in_polygons.md]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import points_in_polygons_common as PC  # noqa: E402
import rasterize_common as R  # noqa: E402
from pcr import _cabi as A  # noqa: E402
from rasterize_time import inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--sides", default="0", help="index sides to time, comma separated; 0: automatic (e.g. 0,512,256)")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    G, n = args.grid, args.points
    m = min(args.sample, n)
    L = A.lib()
    if A.device_count() < 1:
        raise RuntimeError("no HIP device")
    ev = [C.c_void_p() for _ in range(4)]
    for e in ev:
        A.check(L.pcr_hip_event_create(C.byref(e)))

    def elapsed(a, b):
        ms = C.c_float(0.0)
        A.check(L.pcr_hip_event_elapsed_ms(a, b, C.byref(ms)))
        return ms.value

    rng = np.random.default_rng(17)
    x, y = rng.uniform(0.0, float(G), n), rng.uniform(0.0, float(G), n)
    d_x, d_y = A.DeviceBuffer.from_numpy(x), A.DeviceBuffer.from_numpy(y)
    d_out, d_copy_src, d_copy_dst = A.DeviceBuffer(4 * n), A.DeviceBuffer(10 * n), A.DeviceBuffer(10 * n)
    d_band = A.DeviceBuffer(4 * G * G)
    geom = R.Geom(G, G)
    grid = geom.cabi(A)
    events = (C.c_void_p * 2)(ev[0].value, ev[1].value)
    med = statistics.median
    span = lambda v: [round(min(v), 4), round(max(v), 4)]
    rows = []
    for name, polys, side in [(nm, pl, int(sd)) for nm, pl in inputs(G) for sd in args.sides.split(",")]:
        V, Rn, P = len(polys.coords), len(polys.ring_offsets) - 1, polys.P
        t0 = time.perf_counter()
        ix = PC.Index(A, polys, side, side)
        t_build = (time.perf_counter() - t0) * 1e3
        info = ix.info()
        t0 = time.perf_counter()
        ix.upload()
        t_upload = (time.perf_counter() - t0) * 1e3

        def kernel():
            A.check(L.pcr_hip_points_in_polygons(ix.ptr, ix.d_tables.ptr, d_x.ptr, d_y.ptr, n, d_out.ptr, None, events))

        kernel()
        A.check(L.pcr_hip_stream_synchronize(None))
        got = np.empty(m, np.float32)
        A.check(L.pcr_hip_memcpy_d2h(got.ctypes.data, d_out.ptr, 4 * m, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        xs, ys = np.ascontiguousarray(x[:m]), np.ascontiguousarray(y[:m])
        t0 = time.perf_counter()
        want = ix.host(xs, ys, threads=args.host_threads)
        t_host = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name}: the kernel differs from the host twin"
        inside = int((~np.isnan(want)).sum())

        # the cell-resolution route: the label band, once, then NEAREST at the points
        nbytes = C.c_size_t(0)
        A.check(L.pcr_hip_rasterize_work_bytes(V, P, G, G, C.byref(nbytes)))
        d_work = A.DeviceBuffer(nbytes.value)
        plain = A.RasterizeParams()
        A.check(L.pcr_hip_rasterize_polygons(C.byref(grid), *PC.poly_args(polys), C.byref(plain), d_band.ptr, G, d_work.ptr, nbytes.value, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        d_work.free()

        t_kernel, t_copy, t_nearest = [], [], []
        for i in range(args.warmup + args.steps):
            kernel()
            A.check(L.pcr_hip_event_record(ev[2], None))
            A.check(L.pcr_hip_copy_kernel(d_copy_dst.ptr, d_copy_src.ptr, 10 * n // 16 * 16, 1, None))
            A.check(L.pcr_hip_event_record(ev[3], None))
            A.check(L.pcr_hip_stream_synchronize(None))
            k, c = elapsed(ev[0], ev[1]), elapsed(ev[2], ev[3])
            A.check(L.pcr_hip_event_record(ev[2], None))
            A.check(L.pcr_hip_sample_grid(C.byref(grid), d_band.ptr, G, d_x.ptr, d_y.ptr, None, n, A.SAMPLE_NEAREST, d_out.ptr, None))
            A.check(L.pcr_hip_event_record(ev[3], None))
            A.check(L.pcr_hip_stream_synchronize(None))
            if i >= args.warmup:
                t_kernel.append(k)
                t_copy.append(c)
                t_nearest.append(elapsed(ev[2], ev[3]))
        ix.close()
        rows.append({"input": name, "index_side_asked": side, "polygons": P, "vertices": V, "points_inside_of_sample": inside, "sample": m,
                     "index_cols": info["cols"], "index_rows": info["rows"], "index_items": info["items"],
                     "index_listed_edges": info["listed_edges"], "index_bytes": info["bytes"],
                     "kernel_ms": round(med(t_kernel), 4), "kernel_min_max": span(t_kernel),
                     "copy_ms": round(med(t_copy), 4), "copy_min_max": span(t_copy),
                     "kernel_over_copy": round(med(t_kernel) / med(t_copy), 2),
                     "sample_nearest_ms": round(med(t_nearest), 4), "sample_nearest_min_max": span(t_nearest),
                     "kernel_over_sample_nearest": round(med(t_kernel) / med(t_nearest), 2),
                     "index_build_ms": round(t_build, 2), "index_upload_ms": round(t_upload, 3),
                     "host_twin_sample_ms": round(t_host, 2), "host_threads": args.host_threads,
                     "host_twin_scaled_to_all_points_ms": round(t_host * n / m, 1)})
    total = {"points": n, "extent": G, "steps": args.steps, "warmup": args.warmup, "bytes_moved_per_point": 20,
             "equals_host_twin_on_sample": True, "inputs": rows}
    print(json.dumps(total), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"{n} points spread uniformly over a {G} x {G} extent, tested against polygons on one MI355X; the first {m} answers "
                    f"equal to the host twin's bit for bit.  Median of {args.steps} after {args.warmup} warm-ups (min .. max).  The kernel is "
                    f"timed between the two events its call records; each call alternates with the non-temporal copy kernel copying 10 "
                    f"bytes per point (10 read, 10 written: the 20 bytes per point the kernel must move) and with pcr_hip_sample_grid "
                    f"NEAREST on the rasterized {G} x {G} label band, the cell-resolution route.\n\n")
            f.write("| input | index | polygons | vertices | k_points_in_polygons, ms | copy of 20 bytes per point, ms | kernel / copy | "
                    "sample_grid NEAREST on the label band, ms | kernel / NEAREST |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['input']} | {r['index_side_asked'] or 'automatic'} | {r['polygons']} | {r['vertices']} | {r['kernel_ms']:.3f} ({r['kernel_min_max'][0]:.3f} .. "
                        f"{r['kernel_min_max'][1]:.3f}) | {r['copy_ms']:.3f} ({r['copy_min_max'][0]:.3f} .. {r['copy_min_max'][1]:.3f}) | "
                        f"{r['kernel_over_copy']:.2f} | {r['sample_nearest_ms']:.3f} ({r['sample_nearest_min_max'][0]:.3f} .. "
                        f"{r['sample_nearest_min_max'][1]:.3f}) | {r['kernel_over_sample_nearest']:.2f} |\n")
            f.write(f"\n| input | index cols x rows | items | listed edges | table bytes | index build, ms (host, one thread, wall clock) | "
                    f"upload, ms (wall clock) | host twin, {args.host_threads} threads, {m} points, ms | ... scaled to all points, ms |\n"
                    "|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['input']} | {r['index_cols']} x {r['index_rows']} | {r['index_items']} | {r['index_listed_edges']} | "
                        f"{r['index_bytes']} | {r['index_build_ms']:.1f} | {r['index_upload_ms']:.2f} | {r['host_twin_sample_ms']:.1f} | "
                        f"{r['host_twin_scaled_to_all_points_ms']:.0f} |\n")


if __name__ == "__main__":
    main()
