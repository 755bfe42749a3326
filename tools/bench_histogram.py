#!/usr/bin/env python3
"""ms per ingest+finalize of a pipeline with one per-cell histogram beside a Point Count, on C2's shape (50 M uniform points,
4096 x 4096, device-resident cloud and result; values normally distributed inside [lo, hi)).  Prints one JSON line per run.

Timing as in bench.py: every step runs on a fresh pipeline created before the clock starts (scratch arena sized and cube zeroed
at create), W untimed warm-up steps, then K timed steps, each between two device synchronisations; the MEDIAN of the K is
reported.

    python tools/bench_histogram.py [--steps 10] [--warmup 3] [--points 50000000] [--grid 4096] [--bins 32,64]
                                    [--paths binned,direct] [--slabs 8,16,32] [--legs count,hist,percentiles]

Legs:
  count        the Point Count alone -- needs nothing of the histograms: `--legs count` runs on a tree that does not have them
               (the yardstick of profiles/histogram.md)
  hist         Count + one histogram, for every bin count, path and -- on the binned path -- every S (the bin planes an LDS tile
               holds, PCR_HIP_DEBUG_HIST_SLAB); also one profiled step's per-kernel milliseconds
  percentiles  pcr_hip_histogram_percentiles alone (two bands) on a cube an ingest filled, between two events"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
os.environ.setdefault("PCR_REQUIRE_GPU_ENGINE", "1")

import torch  # noqa: E402

import pcr  # noqa: E402

LO, HI = 0.0, 64.0


def device_cloud(n, G, seed):
    c = pcr.PointCloud.create(max(n, 1), pcr.MemoryLocation.Device)
    if c is None:
        raise MemoryError("cannot allocate the device cloud")
    c.add_channel("value", pcr.DataType.Float32)
    c.resize(n)
    ptrs = c.device_ptrs()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    for name in ("x", "y"):
        t = torch.as_tensor(pcr.DeviceArrayView(ptrs[name], (max(n, 1),), "<f8", owner=c), device="cuda")
        t[:n].uniform_(2.0, G - 2.0, generator=gen)
    t = torch.as_tensor(pcr.DeviceArrayView(ptrs["value"], (max(n, 1),), "<f4", owner=c), device="cuda")
    t[:n].normal_((LO + HI) / 2, (HI - LO) / 8, generator=gen).clamp_(LO, HI - 0.01)     # inside [lo, hi): no end-bin pile-up
    torch.cuda.synchronize()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--bins", default="32,64")
    ap.add_argument("--paths", default="binned,direct")
    ap.add_argument("--slabs", default="8,16,32")
    ap.add_argument("--legs", default="count,hist,percentiles")
    args = ap.parse_args()
    G, n = args.grid, args.points
    legs = [s for s in args.legs.split(",") if s]
    cloud = device_cloud(n, G, 42)
    base = {"points": n, "grid": [G, G], "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    def make_pipe(bins, path):
        cfg = pcr.PipelineConfig()
        cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(G), float(G))
        cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
        cfg.grid.compute_dimensions()
        cfg.exec_mode = pcr.ExecutionMode.GPU
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", pcr.ReductionType.Count
        cfg.reductions = [r]
        if bins:
            cfg.histograms = [pcr.HistogramConfig("value", LO, HI, bins, [0.5, 0.95])]
        cfg.result_location = pcr.MemoryLocation.Device
        cfg.scatter_path = {"auto": 0, "direct": 1, "binned": 2}[path]
        cfg.gpu_pool_size_bytes = 24 * n + (64 << 20)
        p = pcr.Pipeline.create(cfg)
        if p is None:
            raise RuntimeError(pcr.pipeline_create_error())
        return p

    def step(p):
        p.ingest(cloud)
        p.finalize()

    def timed(bins, path):
        pipes = [make_pipe(bins, path) for _ in range(args.warmup + args.steps)]
        for p in pipes[:args.warmup]:
            step(p)
        torch.cuda.synchronize()
        ms = []
        for p in pipes[args.warmup:]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(p)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"ms": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                "scatter": pipes[-1].last_scatter()["path"], "lds_tile": list(pipes[-1].last_scatter()["lds_tile"])}

    def kernels(bins, path):
        p = make_pipe(bins, path)
        step(make_pipe(bins, path))
        p.profile_enable(True)
        step(p)
        torch.cuda.synchronize()
        return {name: round(ms, 4) for name, (launches, ms) in p.profile_read(True).items()}

    if "count" in legs:
        print(json.dumps({"metric": "point_count_ms_per_step", **base, **timed(0, "binned")}), flush=True)
    if "hist" in legs:
        for bins in [int(b) for b in args.bins.split(",") if b]:
            for path in [s for s in args.paths.split(",") if s]:
                for slab in ([int(s) for s in args.slabs.split(",") if s] if path == "binned" else [0]):
                    if slab:
                        os.environ["PCR_HIP_DEBUG_HIST_SLAB"] = str(slab)      # read when a pipeline's engine is created
                    out = {"metric": "histogram_ms_per_step", **base, "bins": bins, "path": path, "S": slab or None}
                    out.update(timed(bins, path))
                    out["kernels_ms"] = kernels(bins, path)
                    print(json.dumps(out), flush=True)
        os.environ.pop("PCR_HIP_DEBUG_HIST_SLAB", None)
    if "percentiles" in legs:
        from pcr import _cabi as A
        L = A.lib()
        for bins in [int(b) for b in args.bins.split(",") if b]:
            p = make_pipe(bins, "binned")
            p.ingest(cloud)
            p.synchronize()
            # a cube of the same content in memory of our own: Pipeline.histogram is a host copy
            cube = torch.from_numpy(p.histogram(0).view("int32")).cuda()
            outs = torch.empty((2, G, G), dtype=torch.float32, device="cuda")
            g = A.make_grid((0, 0, G, G), dims=(G, G))
            q = (C.c_float * 2)(0.5, 0.95)
            ptrs = (C.c_void_p * 2)(outs[0].data_ptr(), outs[1].data_ptr())
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            ms = []
            for k in range(args.warmup + args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                A.check(L.pcr_hip_histogram_percentiles(C.byref(g), C.c_void_p(cube.data_ptr()), bins, LO, (HI - LO) / bins, 2, q, ptrs,
                                                        stream))
                b.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ms.append(a.elapsed_time(b))
            print(json.dumps({"metric": "histogram_percentiles_ms", **base, "bins": bins, "bands": 2,
                              "ms": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                              "cube_gb": round(bins * G * G * 4 / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
