#!/usr/bin/env python3
"""What the overview pyramid costs (profiles/overviews.md).  Prints one JSON line.

Leg "kernel": one G x G float32 band in HBM (default 16384: 1 GiB) and the levels of the reference's rule (six at 16384),
pcr_hip_downsample2 against a device-to-device hipMemcpyAsync of the same band -- which reads what the pyramid reads and
writes three times what it writes.  Both in one process, alternating, each call between two device events: W warm-ups,
then the MEDIAN of K timed calls.  GB/s over the bytes the algorithm needs: 4 B read + 4/3 B written per cell for the
pyramid (the exact sum of the level sizes is used), 8 B per cell for the copy.  The levels are checked first: level 1's
top rows and levels 4.. (from the device's level 3) against the NumPy model, bit for bit.

Leg "file": wall time of Pipeline.finalize() with output_path set on a P x P grid with Sum + Average + Count (default 4096:
C2's shape), write_cog off and on, alternating, fresh pipelines, median of R; and, per repetition, the parts on their own
("parts"): the levels built on the device, copied to the host, the writer without and with ready-made levels, the levels built
by the host loop.

    python tools/bench_overviews.py [--grid 16384] [--steps 20] [--warmup 3] [--file-grid 4096] [--file-reps 3]
                                    [--legs kernel,file] [--mode average|nearest] [--hold]

--hold: one warm-up and one timed call of the pyramid and nothing else -- what a kernel trace wants."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("PCR_REQUIRE_GPU_ENGINE", "1")

import numpy as np  # noqa: E402

import pcr  # noqa: E402
from pcr import _cabi as A  # noqa: E402


def model_down(src, mode):
    import overviews_common as M
    return M.down(src, mode)


def kernel_leg(G, steps, warmup, mode, hold):
    L = A.lib()
    if A.device_count() < 1:
        raise RuntimeError("no HIP device")
    rng = np.random.default_rng(1)
    block = rng.normal(0.0, 100.0, (1024, min(G, 1024))).astype(np.float32)
    block[rng.uniform(size=block.shape) < 0.2] = np.nan
    band = np.tile(block, ((G + 1023) // 1024, (G + block.shape[1] - 1) // block.shape[1]))[:G, :G]
    band = np.ascontiguousarray(band)
    src = A.DeviceBuffer.from_numpy(band)
    levels = 0
    while min(G, G) // (2 << levels) >= 256:
        levels += 1
    if levels == 0:
        raise ValueError("--grid too small for the reference's rule (needs min(W, H) / 2 >= 256)")
    shapes = [((G + (1 << k) - 1) >> k,) * 2 for k in range(1, levels + 1)]
    bufs = [A.DeviceBuffer(4 * s[0] * s[1]) for s in shapes]
    ptrs = (C.c_void_p * levels)(*[b.ptr.value for b in bufs])
    m = 0 if mode == "average" else 1
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

    def pyramid():
        A.check(L.pcr_hip_downsample2(src.ptr, G, G, G, ptrs, levels, m, None))

    if hold:
        timed(pyramid)
        return {"grid": G, "levels": levels, "pyramid_ms_once": round(timed(pyramid), 4)}

    # correctness at this size before any timing
    pyramid()
    A.check(L.pcr_hip_stream_synchronize(None))
    rows = min(G, 2048)
    l1 = bufs[0].to_numpy(np.float32, shapes[0])
    want = model_down(band[:rows], mode)
    assert np.array_equal(l1[:rows // 2].view(np.uint32), want.view(np.uint32)), "level 1 differs from the model"
    if levels >= 4:
        prev = bufs[2].to_numpy(np.float32, shapes[2])
        for k in range(3, levels):
            prev = model_down(prev, mode)
            got = bufs[k].to_numpy(np.float32, shapes[k])
            assert np.array_equal(got.view(np.uint32), prev.view(np.uint32)), f"level {k + 1} differs from the model"
    del l1

    copy_dst = A.DeviceBuffer(band.nbytes)

    def copy():
        A.check(L.pcr_hip_memcpy_d2d(copy_dst.ptr, src.ptr, band.nbytes, None))

    t_pyr, t_copy = [], []
    for i in range(warmup + steps):
        a, b = timed(pyramid), timed(copy)
        if i >= warmup:
            t_pyr.append(a)
            t_copy.append(b)
    pyr_bytes = band.nbytes + sum(4 * s[0] * s[1] for s in shapes)
    mp, mc = statistics.median(t_pyr), statistics.median(t_copy)
    return {"grid": G, "levels": levels, "mode": mode, "steps": steps, "warmup": warmup,
            "pyramid_ms": round(mp, 4), "pyramid_ms_min_max": [round(min(t_pyr), 4), round(max(t_pyr), 4)],
            "copy_d2d_ms": round(mc, 4), "copy_d2d_ms_min_max": [round(min(t_copy), 4), round(max(t_copy), 4)],
            "pyramid_bytes": pyr_bytes, "pyramid_GBps": round(pyr_bytes / mp / 1e6, 1),
            "copy_bytes": 2 * band.nbytes, "copy_GBps": round(2 * band.nbytes / mc / 1e6, 1),
            "pyramid_over_copy": round(mp / mc, 3), "levels_checked_against_model": True}


def file_leg(P, reps, n_points):
    rng = np.random.default_rng(2)
    cloud = pcr.PointCloud.create(n_points)
    cloud.set_x_array(rng.uniform(1.0, P - 1.0, n_points))
    cloud.set_y_array(rng.uniform(1.0, P - 1.0, n_points))
    cloud.add_channel("value", pcr.DataType.Float32)
    cloud.set_channel_array_f32("value", rng.uniform(0.0, 1.0, n_points).astype(np.float32))
    times = {False: [], True: []}
    sizes, parts = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(reps + 1):                                   # rep 0: warm-up
            for cog in (False, True):
                cfg = pcr.PipelineConfig()
                cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(P), float(P))
                cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
                cfg.grid.compute_dimensions()
                cfg.exec_mode = pcr.ExecutionMode.GPU
                specs = []
                for t in (pcr.ReductionType.Sum, pcr.ReductionType.Average, pcr.ReductionType.Count):
                    r = pcr.ReductionSpec()
                    r.value_channel, r.type = "value", t
                    specs.append(r)
                cfg.reductions = specs
                cfg.output_path, cfg.write_cog = os.path.join(tmp, f"f{int(cog)}.tif"), cog
                pipe = pcr.Pipeline.create(cfg)
                if pipe is None or pipe.engine() != "hip":
                    raise RuntimeError("no HIP pipeline: " + pcr.pipeline_create_error())
                pipe.ingest(cloud)
                pipe.synchronize()
                t0 = time.perf_counter()
                pipe.finalize()
                dt = time.perf_counter() - t0
                if rep:
                    times[cog].append(dt * 1e3)
                sizes[cog] = (os.path.getsize(cfg.output_path), pcr.read_geotiff_overviews(cfg.output_path))
                if cog and rep:                                       # where the difference goes: the parts on their own
                    res, scratch = pipe.result(), os.path.join(tmp, "part.tif")
                    t0 = time.perf_counter()
                    dev = res.to(pcr.MemoryLocation.Device)
                    t1 = time.perf_counter()
                    lv = pcr.build_overviews(dev, -1)                 # (allocates the levels, launches, synchronises)
                    t2 = time.perf_counter()
                    host_lv = [g.to_host() for g in lv]
                    t3 = time.perf_counter()
                    pcr.write_geotiff(scratch, res, cfg.grid, pcr.GeoTiffOptions())
                    t4 = time.perf_counter()
                    pcr.write_geotiff(scratch, res, cfg.grid, pcr.GeoTiffOptions(), overviews=host_lv)
                    t5 = time.perf_counter()
                    host_built = pcr.build_overviews(res, -1)
                    t6 = time.perf_counter()
                    parts.append({"build_on_device_ms": round((t2 - t1) * 1e3, 1), "levels_to_host_ms": round((t3 - t2) * 1e3, 1),
                                  "write_plain_ms": round((t4 - t3) * 1e3, 1), "write_with_levels_ms": round((t5 - t4) * 1e3, 1),
                                  "build_on_host_ms": round((t6 - t5) * 1e3, 1)})
                    del dev, lv, host_lv, host_built
                del pipe
    return {"grid": P, "bands": 3, "points": n_points, "reps": reps,
            "finalize_to_file_ms": round(statistics.median(times[False]), 1),
            "finalize_to_file_cog_ms": round(statistics.median(times[True]), 1),
            "all_ms": {"plain": [round(t, 1) for t in times[False]], "cog": [round(t, 1) for t in times[True]]},
            "file_bytes": sizes[False][0], "file_bytes_cog": sizes[True][0], "levels": sizes[True][1], "parts": parts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--file-grid", type=int, default=4096)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--file-points", type=int, default=20_000_000)
    ap.add_argument("--legs", default="kernel,file")
    ap.add_argument("--mode", default="average", choices=["average", "nearest"])
    ap.add_argument("--hold", action="store_true")
    args = ap.parse_args()
    out = {}
    legs = args.legs.split(",")
    if "kernel" in legs:
        out["kernel"] = kernel_leg(args.grid, args.steps, args.warmup, args.mode, args.hold)
    if "file" in legs and not args.hold:
        out["file"] = file_leg(args.file_grid, args.file_reps, args.file_points)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
