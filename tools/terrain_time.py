#!/usr/bin/env python3
"""What pcr_hip_terrain costs (profiles/terrain.md).  Prints one JSON line per case.

One G x G float32 band in HBM (default 4096), a rolling surface with 5 % NaN cells: one product at a time, hillshade + slope
+ aspect, and all seven, each next to pcr_hip_copy_kernel (non-temporal) on the same band.  Both in one process, alternating,
each call between two device events: W warm-ups, then the MEDIAN, minimum and maximum of K timed calls.  The copy kernel moves
two bands (one read, one written), a launch with k products moves 1 + k: `per_band_ratio` is the kernel's time over the copy
kernel's scaled to the same bytes, kernel_ms / (copy_ms * (1 + k) / 2).  Before any timing the device result of every case is
compared bit for bit with the host loop on the whole band.

    python tools/terrain_time.py [--grid 4096] [--steps 10] [--warmup 2] [--md profiles/terrain.md]

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
from pcr import _pcr  # noqa: E402

P = pcr.TerrainProduct
NAMES = ["slope", "slope_percent", "aspect", "hillshade", "tri", "tpi", "roughness"]
ALL = [P.SlopeDegrees, P.SlopePercent, P.Aspect, P.Hillshade, P.TRI, P.TPI, P.Roughness]


def band(G):
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:G, 0:G].astype(np.float32)
    z = 100.0 + 8.0 * np.sin(xx / 31.0) * np.cos(yy / 27.0) + 0.04 * xx + rng.normal(0.0, 0.03, (G, G)).astype(np.float32)
    z = z.astype(np.float32)
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
    outs = [A.DeviceBuffer(4 * G * G) for _ in range(7)]
    copy_dst = A.DeviceBuffer(4 * G * G)
    sin_alt, ls, lc = pcr.terrain_light()

    def measure(products, edges):
        k = len(products)
        ids = (C.c_int * k)(*[int(p) for p in products])
        dsts = (C.c_void_p * k)(*[o.ptr.value for o in outs[:k]])
        strides = (C.c_int64 * k)(*([G] * k))

        def run():
            A.check(L.pcr_hip_terrain(src.ptr, G, G, G, k, ids, dsts, strides, 1.0, -1.0, 1.0, edges, sin_alt, ls, lc, None))

        def copy():
            A.check(L.pcr_hip_copy_kernel(copy_dst.ptr, src.ptr, 4 * G * G, 1, None))

        run()
        A.check(L.pcr_hip_stream_synchronize(None))
        spec = pcr.TerrainSpec()
        spec.compute_edges = bool(edges)
        want = np.array(_pcr._terrain_host(z, list(products), spec, 1.0, -1.0, 0))
        for j in range(k):
            got = outs[j].to_numpy(np.float32, (G, G))
            assert np.array_equal(got.view(np.uint32), want[j].view(np.uint32)), f"{NAMES[int(products[j])]}: differs from the host loop"
        t_run, t_copy = [], []
        for i in range(args.warmup + args.steps):
            a, b = timed(run), timed(copy)
            if i >= args.warmup:
                t_run.append(a)
                t_copy.append(b)
        mr, mc = statistics.median(t_run), statistics.median(t_copy)
        return {"grid": G, "products": [NAMES[int(p)] for p in products], "edges": edges, "steps": args.steps, "warmup": args.warmup,
                "kernel_ms": round(mr, 4), "kernel_ms_min_max": [round(min(t_run), 4), round(max(t_run), 4)],
                "copy_kernel_ms": round(mc, 4), "copy_kernel_ms_min_max": [round(min(t_copy), 4), round(max(t_copy), 4)],
                "bands_moved": 1 + k, "per_band_ratio": round(mr / (mc * (1 + k) / 2.0), 2), "equals_host_loop": True}

    rows = []
    for products, edges in [([p], 0) for p in ALL] + [([P.Hillshade, P.SlopeDegrees, P.Aspect], 0), (ALL, 0), (ALL, 1)]:
        row = measure(products, edges)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| products ({G} x {G}) | edges | kernel ms (min .. max) | copy kernel ms | bands moved (1 + k) | kernel / copy per band moved |\n"
                    "|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {' + '.join(r['products']) if len(r['products']) < 7 else 'all seven'} | {r['edges']} | {r['kernel_ms']:.3f} "
                        f"({r['kernel_ms_min_max'][0]:.3f} .. {r['kernel_ms_min_max'][1]:.3f}) | {r['copy_kernel_ms']:.3f} | "
                        f"{r['bands_moved']} | {r['per_band_ratio']:.2f} |\n")


if __name__ == "__main__":
    main()
