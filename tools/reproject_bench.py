#!/usr/bin/env python3
"""Times pcr_hip_transform_xy (csrc/reproject.hip) on N device points, out of place, with HIP events: warm-up launches
first, then the median of --runs launches, for 4326 -> 32618 (geographic -> UTM) and 32617 -> 32618 (zone to zone).
Prints one JSON line per pair: ms, Gpts/s and the effective bandwidth (32 B per point: x, y read, x, y written).

    python tools/reproject_bench.py [--points 50000000] [--runs 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import torch
    import pcr
    from pcr import _cabi as A

    L = A.lib()
    n = a.points
    g = torch.Generator(device="cuda").manual_seed(1)
    lon = -75.0 + (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 0.5) * 12.0
    lat = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 0.5) * 160.0
    pairs = [(4326, 32618, lon, lat)]
    ux, uy = pcr.transform_xy(4326, 32617, lon, lat)
    pairs.append((32617, 32618, ux, uy))
    ox, oy = torch.empty_like(lon), torch.empty_like(lat)
    stream = torch.cuda.current_stream().cuda_stream
    for src, dst, x, y in pairs:
        ds, dd = A.CrsDesc(), A.CrsDesc()
        A.check(L.pcr_hip_crs_from_epsg(src, C.byref(ds)))
        A.check(L.pcr_hip_crs_from_epsg(dst, C.byref(dd)))

        def launch():
            A.check(L.pcr_hip_transform_xy(C.byref(ds), C.byref(dd), x.data_ptr(), y.data_ptr(), ox.data_ptr(), oy.data_ptr(),
                                           n, stream))
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        nan = int(torch.isnan(ox).sum().item())
        print(json.dumps({"pair": f"{src}->{dst}", "points": n, "ms": round(ms, 4), "min_ms": round(min(times), 4),
                          "gpts_per_s": round(n / ms / 1e6, 3), "eff_tb_per_s": round(32 * n / ms / 1e9, 3),
                          "runs": a.runs, "nan_points": nan}), flush=True)


if __name__ == "__main__":
    main()
