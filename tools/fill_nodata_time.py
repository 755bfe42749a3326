#!/usr/bin/env python3
"""What pcr_hip_fill_nodata costs (profiles/fill_nodata.md).  Prints one JSON line per case.

One G x G float32 band in HBM (default 4096) and three kinds of band -- without a hole, with 5 % isolated holes, with 30 %
holes in blobs -- at R = 4, 16, 32, each next to pcr_hip_copy_kernel (non-temporal) moving the same 8 B per cell.  Both in one
process, alternating, each call between two device events: W warm-ups, then the MEDIAN of K timed calls.  Before any timing the
top-left corner of the result is checked bit for bit against the host fill of that corner.

    python tools/fill_nodata_time.py [--grid 4096] [--steps 10] [--warmup 2] [--radii 4,16,32] [--md profiles/fill_nodata.md]

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

import pcr  # noqa: E402
from pcr import _cabi as A  # noqa: E402


def bands(G):
    rng = np.random.default_rng(1)
    base = rng.normal(100.0, 30.0, (G, G)).astype(np.float32)
    iso = base.copy()
    iso[rng.uniform(size=(G, G)) < 0.05] = np.nan
    # blobs: discs of radius 8..40 dropped until 30 % of the cells are holes
    blob = base.copy()
    yy, xx = np.mgrid[-40:41, -40:41]
    mask = np.zeros((G, G), bool)
    while mask.mean() < 0.30:
        for _ in range(max(1, G * G // 40000)):
            r = int(rng.integers(8, 41))
            cy, cx = int(rng.integers(40, G - 40)), int(rng.integers(40, G - 40))
            mask[cy - 40:cy + 41, cx - 40:cx + 41] |= yy * yy + xx * xx <= r * r
    blob[mask] = np.nan
    return [("hole-free", base), ("5 % isolated holes", iso), ("30 % holes in blobs", blob)]


def host_fill(a, R):
    b = pcr.BandDesc()
    b.name = "v"
    g = pcr.Grid.create(a.shape[1], a.shape[0], [b])
    g.set_band_array(0, a)
    return np.array(pcr.fill_nodata(g, R).band_array(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radii", default="4,16,32")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    G = args.grid
    radii = [int(r) for r in args.radii.split(",")]
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

    rows = []
    dst = A.DeviceBuffer(4 * G * G)
    copy_dst = A.DeviceBuffer(4 * G * G)
    for name, band in bands(G):
        src = A.DeviceBuffer.from_numpy(band)
        holes = float(np.isnan(band).mean())
        for R in radii:
            def fill():
                A.check(L.pcr_hip_fill_nodata(src.ptr, dst.ptr, G, G, G, G, R, None))

            def copy():
                A.check(L.pcr_hip_copy_kernel(copy_dst.ptr, src.ptr, 4 * G * G, 1, None))

            fill()
            A.check(L.pcr_hip_stream_synchronize(None))
            n = min(G, 256)
            got = dst.to_numpy(np.float32, (G, G))[:n, :n]
            m = min(G, n + R)
            want = host_fill(np.ascontiguousarray(band[:m, :m]), R)[:n, :n]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name} R={R}: differs from the host fill"
            t_fill, t_copy = [], []
            for i in range(args.warmup + args.steps):
                a, b = timed(fill), timed(copy)
                if i >= args.warmup:
                    t_fill.append(a)
                    t_copy.append(b)
            mf, mc = statistics.median(t_fill), statistics.median(t_copy)
            row = {"grid": G, "band": name, "hole_fraction": round(holes, 4), "radius": R, "steps": args.steps, "warmup": args.warmup,
                   "fill_ms": round(mf, 4), "fill_ms_min_max": [round(min(t_fill), 4), round(max(t_fill), 4)],
                   "copy_kernel_ms": round(mc, 4), "copy_kernel_ms_min_max": [round(min(t_copy), 4), round(max(t_copy), 4)],
                   "fill_GBps": round(8.0 * G * G / mf / 1e6, 1), "copy_GBps": round(8.0 * G * G / mc / 1e6, 1),
                   "fill_over_copy": round(mf / mc, 2), "checked_against_host_fill": True}
            print(json.dumps(row), flush=True)
            rows.append(row)
        src.free()
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| band ({G} x {G}) | holes | R | fill ms (min .. max) | copy kernel ms | fill / copy |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['band']} | {100 * r['hole_fraction']:.1f} % | {r['radius']} | {r['fill_ms']:.3f} "
                        f"({r['fill_ms_min_max'][0]:.3f} .. {r['fill_ms_min_max'][1]:.3f}) | {r['copy_kernel_ms']:.3f} | "
                        f"{r['fill_over_copy']:.2f} |\n")


if __name__ == "__main__":
    main()
