#!/usr/bin/env python3
"""What burning polygons into a label band costs (profiles/rasterize.md).  Prints one JSON line.

One G x G grid (default 4096), unit cells, three polygon sets:
  plots      10 000 disjoint 32-gons of about 11 cells radius on a lattice
  stands     a jittered partition of the grid into about 2 000 polygons of about 200 vertices with shared edges
  one        one polygon of 100 000 vertices covering most of the grid
For each the band the kernels make is first compared bit for bit with the host twin's.  Then K timed calls after W warm-ups,
each pcr_hip_rasterize_polygons alternating with pcr_hip_copy_kernel (non-temporal) moving the bytes of the output band: the two
kernels between the events the call records around them (pcr_hip_rasterize_params.events), the copy between two events, the
whole call (host preparation, upload, kernels, synchronise) by the wall clock.  Beside them the host twin on the same input and
the upload of a finished band from pageable host memory, which together are the route set_zones(name, grid) takes.

    python tools/rasterize_time.py [--grid 4096] [--steps 10] [--warmup 2] [--md profiles/rasterize.md]

--md: also writes the table as Markdown (the measured part of the profile; the discussion under it is written by hand)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import rasterize_common as R  # noqa: E402
from pcr import _cabi as A  # noqa: E402


def inputs(G):
    n = max(1, round(100 * G / 4096))
    pitch = G / n
    plots = R.Polys([[R.ngon((i + 0.5) * pitch + 0.13, (j + 0.5) * pitch + 0.29, 11.0 * min(1.0, pitch / 40.96), 32)]
                     for j in range(n) for i in range(n)])
    m = max(1, round(45 * G / 4096))
    stands = R.Polys(R.partition(0.0, 0.0, float(G), float(G), m, m, seed=4, wiggle=49, amp=0.012))
    rng = np.random.default_rng(6)
    a = 2.0 * math.pi * np.arange(100_000) / 100_000
    rad = G * (0.40 + 0.05 * np.sin(9 * a)) + rng.uniform(-0.002 * G, 0.002 * G, len(a))
    one = R.Polys([[np.stack([G / 2 + rad * np.cos(a), G / 2 + rad * np.sin(a)], axis=1)]])
    return [("plots", plots), ("stands", stands), ("one", one)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    G = args.grid
    band_bytes = 4 * G * G
    L = A.lib()
    if A.device_count() < 1:
        raise RuntimeError("no HIP device")
    ev = [C.c_void_p() for _ in range(5)]
    for e in ev:
        A.check(L.pcr_hip_event_create(C.byref(e)))

    def elapsed(a, b):
        ms = C.c_float(0.0)
        A.check(L.pcr_hip_event_elapsed_ms(a, b, C.byref(ms)))
        return ms.value

    geom = R.Geom(G, G)
    grid = geom.cabi(A)
    d_out, d_copy = A.DeviceBuffer(band_bytes), A.DeviceBuffer(band_bytes)
    rows = []
    for name, polys in inputs(G):
        V, Rn, P = len(polys.coords), len(polys.ring_offsets) - 1, polys.P
        args_ = (polys.coords.ctypes.data, V, polys.ring_offsets.ctypes.data, Rn, polys.polygon_offsets.ctypes.data, P, None)
        nbytes = C.c_size_t(0)
        A.check(L.pcr_hip_rasterize_work_bytes(V, P, G, G, C.byref(nbytes)))
        d_work = A.DeviceBuffer(nbytes.value)
        plain = A.RasterizeParams()
        want = np.zeros((G, G), np.float32)

        def host():
            t0 = time.perf_counter()
            A.check(L.pcr_hip_rasterize_polygons_host(C.byref(grid), *args_, C.byref(plain), want.ctypes.data, G))
            return (time.perf_counter() - t0) * 1e3

        def device(p):
            t0 = time.perf_counter()
            A.check(L.pcr_hip_rasterize_polygons(C.byref(grid), *args_, C.byref(p), d_out.ptr, G, d_work.ptr, nbytes.value, None))
            A.check(L.pcr_hip_stream_synchronize(None))
            return (time.perf_counter() - t0) * 1e3

        def upload():
            t0 = time.perf_counter()
            A.check(L.pcr_hip_memcpy_h2d(d_copy.ptr, want.ctypes.data, band_bytes, None))
            A.check(L.pcr_hip_stream_synchronize(None))
            return (time.perf_counter() - t0) * 1e3

        t_host = [host() for _ in range(3)]
        device(plain)
        got = d_out.to_numpy(np.float32, (G, G))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name}: the kernels differ from the host twin"
        labelled = int((~np.isnan(want)).sum())

        timed = A.RasterizeParams(events=(ev[0].value, ev[1].value, ev[2].value))
        fill, values, copy, call, up = [], [], [], [], []
        for i in range(args.warmup + args.steps):
            wall = device(timed)
            A.check(L.pcr_hip_event_record(ev[3], None))
            A.check(L.pcr_hip_copy_kernel(d_copy.ptr, d_out.ptr, band_bytes, 1, None))
            A.check(L.pcr_hip_event_record(ev[4], None))
            t_copy = elapsed(ev[3], ev[4])
            t_up = upload()
            if i >= args.warmup:
                fill.append(elapsed(ev[0], ev[1]))
                values.append(elapsed(ev[1], ev[2]))
                copy.append(t_copy)
                call.append(wall)
                up.append(t_up)
        d_work.free()
        med = statistics.median
        span = lambda v: [round(min(v), 4), round(max(v), 4)]
        rows.append({"input": name, "polygons": P, "vertices": V, "cells_labelled": labelled, "work_bytes": nbytes.value,
                     "k_poly_fill_ms": round(med(fill), 4), "k_poly_fill_min_max": span(fill),
                     "k_poly_values_ms": round(med(values), 4), "k_poly_values_min_max": span(values),
                     "copy_ms": round(med(copy), 4), "copy_min_max": span(copy),
                     "fill_over_copy": round(med(fill) / med(copy), 2), "values_over_copy": round(med(values) / med(copy), 2),
                     "device_call_wall_ms": round(med(call), 3), "device_call_min_max": span(call),
                     "host_twin_ms": round(med(t_host), 2), "host_twin_min_max": span(t_host),
                     "upload_ms": round(med(up), 3), "upload_min_max": span(up)})
    total = {"grid": G, "steps": args.steps, "warmup": args.warmup, "band_bytes": band_bytes, "equals_host_twin": True, "inputs": rows}
    print(json.dumps(total), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"Polygons burnt into a {G} x {G} Float32 band ({band_bytes} bytes) on one MI355X; every band equal to the host "
                    f"twin's bit for bit.  Median of {args.steps} after {args.warmup} warm-ups (min .. max); each call alternates with the "
                    f"non-temporal copy kernel moving the bytes of the band.  Kernel times are between the events the call records "
                    f"around its kernels; the device call and the host twin are by the wall clock.\n\n")
            f.write("| input | polygons | vertices | cells labelled | k_poly_fill, ms | k_poly_values, ms | copy of the band, ms | fill / copy | "
                    "values / copy |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['input']} | {r['polygons']} | {r['vertices']} | {r['cells_labelled']} | {r['k_poly_fill_ms']:.3f} "
                        f"({r['k_poly_fill_min_max'][0]:.3f} .. {r['k_poly_fill_min_max'][1]:.3f}) | {r['k_poly_values_ms']:.3f} "
                        f"({r['k_poly_values_min_max'][0]:.3f} .. {r['k_poly_values_min_max'][1]:.3f}) | {r['copy_ms']:.3f} "
                        f"({r['copy_min_max'][0]:.3f} .. {r['copy_min_max'][1]:.3f}) | {r['fill_over_copy']:.2f} | {r['values_over_copy']:.2f} |\n")
            f.write("\n| input | device call, wall clock, ms (host preparation, upload, kernels, synchronise) | host twin, ms | upload of a "
                    "finished band from pageable memory, ms | host twin + upload: the route of set_zones(name, grid), ms |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['input']} | {r['device_call_wall_ms']:.2f} ({r['device_call_min_max'][0]:.2f} .. {r['device_call_min_max'][1]:.2f}) | "
                        f"{r['host_twin_ms']:.1f} ({r['host_twin_min_max'][0]:.1f} .. {r['host_twin_min_max'][1]:.1f}) | {r['upload_ms']:.2f} "
                        f"({r['upload_min_max'][0]:.2f} .. {r['upload_min_max'][1]:.2f}) | {r['host_twin_ms'] + r['upload_ms']:.1f} |\n")


if __name__ == "__main__":
    main()
