#!/usr/bin/env python3
"""What pcr_hip_ground_filter costs (profiles/ground_filter.md).  Prints one JSON line per case.

One G x G float32 band in HBM (default 4096): the Min band of a synthetic terrain (rolling ground, boxes on it) with 20 % NaN
cells and the same band without holes, through the exponential schedule to 16 (PDAL's default, 5 levels) and to 64 (7 levels)
and the linear schedule to 16 (16 levels), each next to pcr_hip_copy_kernel (non-temporal) on the same band.  Both in one
process, alternating, each call between two device events: W warm-ups, then the MEDIAN, minimum and maximum of K timed calls.
Then single-level calls at R = 1, 2, 4, ... 64 on the band without holes: what a level costs as the apron grows.  Before any
timing the device result of every case is compared bit for bit with the host loop on the whole band.

    python tools/ground_filter_time.py [--grid 4096] [--steps 10] [--warmup 2] [--md profiles/ground_filter.md]

--md: also writes the tables as Markdown."""
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


def bands(G):
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:G, 0:G].astype(np.float32)
    z = 100.0 + 8.0 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 0.004 * xx + rng.normal(0.0, 0.03, (G, G)).astype(np.float32)
    z = z.astype(np.float32)
    for _ in range(G * G // 20000):                                  # buildings and trees: 2 .. 25 m up, 3 .. 40 cells a side
        r, c = int(rng.integers(0, G)), int(rng.integers(0, G))
        z[r:r + int(rng.integers(3, 41)), c:c + int(rng.integers(3, 41))] += np.float32(rng.uniform(2.0, 25.0))
    holes = z.copy()
    holes[rng.uniform(size=(G, G)) < 0.20] = np.nan
    return [("20 % NaN", holes), ("no holes", z)]


def schedules():
    out = []
    for name, exponential, max_radius in (("exponential to 16", True, 16), ("exponential to 64", True, 64), ("linear to 16", False, 16)):
        s = pcr.GroundFilterSpec()
        s.exponential, s.max_radius_cells = exponential, max_radius
        out.append((name,) + tuple(pcr.ground_filter_levels(s, 1.0)))
    return out


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

    need = C.c_size_t(0)
    A.check(L.pcr_hip_ground_filter_work_bytes(G, G, C.byref(need)))
    work = A.DeviceBuffer(need.value)
    dst = A.DeviceBuffer(4 * G * G)
    copy_dst = A.DeviceBuffer(4 * G * G)

    def measure(src, band, radii, thresholds, what):
        rad = (C.c_int * len(radii))(*radii)
        thr = (C.c_float * len(radii))(*thresholds)

        def run():
            A.check(L.pcr_hip_ground_filter(src.ptr, dst.ptr, G, G, G, G, len(radii), rad, thr, work.ptr, need.value, None))

        def copy():
            A.check(L.pcr_hip_copy_kernel(copy_dst.ptr, src.ptr, 4 * G * G, 1, None))

        run()
        A.check(L.pcr_hip_stream_synchronize(None))
        got = dst.to_numpy(np.float32, (G, G))
        want = _pcr._ground_filter_host(band, list(radii), [float(t) for t in thresholds])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: differs from the host loop"
        t_run, t_copy = [], []
        for i in range(args.warmup + args.steps):
            a, b = timed(run), timed(copy)
            if i >= args.warmup:
                t_run.append(a)
                t_copy.append(b)
        mr, mc = statistics.median(t_run), statistics.median(t_copy)
        return {"grid": G, "levels": len(radii), "max_radius": radii[-1], "steps": args.steps, "warmup": args.warmup,
                "filter_ms": round(mr, 4), "filter_ms_min_max": [round(min(t_run), 4), round(max(t_run), 4)],
                "ms_per_level": round(mr / len(radii), 4),
                "copy_kernel_ms": round(mc, 4), "copy_kernel_ms_min_max": [round(min(t_copy), 4), round(max(t_copy), 4)],
                "filter_over_copy": round(mr / mc, 2), "level_over_copy": round(mr / len(radii) / mc, 2),
                "removed_fraction": round(float(np.isnan(got).mean() - np.isnan(band).mean()), 4), "equals_host_loop": True}

    rows, singles = [], []
    for name, band in bands(G):
        src = A.DeviceBuffer.from_numpy(band)
        for sched, radii, thresholds in schedules():
            row = dict(band=name, schedule=sched, **measure(src, band, radii, thresholds, f"{name}, {sched}"))
            print(json.dumps(row), flush=True)
            rows.append(row)
        if name == "no holes":
            for R in (1, 2, 4, 8, 16, 32, 64):
                row = dict(band=name, schedule=f"one level, R = {R}", **measure(src, band, [R], [0.5], f"{name}, R={R}"))
                print(json.dumps(row), flush=True)
                singles.append(row)
        src.free()
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| band ({G} x {G}) | schedule | levels | filter ms (min .. max) | ms per level | copy kernel ms | level / copy |\n"
                    "|---|---|---|---|---|---|---|\n")
            for r in rows + singles:
                f.write(f"| {r['band']} | {r['schedule']} | {r['levels']} | {r['filter_ms']:.3f} ({r['filter_ms_min_max'][0]:.3f} .. "
                        f"{r['filter_ms_min_max'][1]:.3f}) | {r['ms_per_level']:.3f} | {r['copy_kernel_ms']:.3f} | {r['level_over_copy']:.2f} |\n")


if __name__ == "__main__":
    main()
