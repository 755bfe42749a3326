#!/usr/bin/env python3
"""ms per ingest+finalize of a pipeline with one per-cell stats entry beside a Point Min, on C2's shape (50 M uniform points,
4096 x 4096, device-resident cloud and result; values normally distributed around 32 with sigma 8, stepped at a centimetre).
Prints one JSON line per run.

Timing as in bench.py: every step runs on a fresh pipeline created before the clock starts (scratch arena sized and the three
planes zeroed at create), W untimed warm-up steps, then K timed steps, each between two device synchronisations; the MEDIAN of
the K is reported, with the minimum and the maximum.

    python tools/bench_cell_stats.py [--steps 10] [--warmup 3] [--points 50000000] [--grid 4096]
                                     [--paths binned,direct] [--legs min,stat] [--repeat 1]

Legs:
  min    the Point Min alone -- needs nothing of the cell stats: `--legs min` runs on a tree that does not have them (the
         yardstick of profiles/cell_stats.md); --repeat R measures it R times over, for the run-to-run spread
  stat   Min + one entry (Mean and StdDev), for every path; also one profiled step's per-kernel milliseconds"""
import argparse
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
    t[:n].normal_(32.0, 8.0, generator=gen)
    torch.cuda.synchronize()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--paths", default="binned,direct")
    ap.add_argument("--legs", default="min,stat")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    G, n = args.grid, args.points
    legs = [s for s in args.legs.split(",") if s]
    cloud = device_cloud(n, G, 42)
    base = {"points": n, "grid": [G, G], "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    if args.tag:
        base["tag"] = args.tag

    def make_pipe(with_stats, path):
        cfg = pcr.PipelineConfig()
        cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(G), float(G))
        cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
        cfg.grid.compute_dimensions()
        cfg.exec_mode = pcr.ExecutionMode.GPU
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", pcr.ReductionType.Min
        cfg.reductions = [r]
        if with_stats:
            cfg.cell_stats = [pcr.CellStatsConfig("value", origin=0.0, resolution=0.01,
                                                  products=[pcr.CellStat.Mean, pcr.CellStat.StdDev], ddof=0)]
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

    def timed(with_stats, path):
        pipes = [make_pipe(with_stats, path) for _ in range(args.warmup + args.steps)]
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

    def kernels(with_stats, path):
        p = make_pipe(with_stats, path)
        step(make_pipe(with_stats, path))
        p.profile_enable(True)
        step(p)
        torch.cuda.synchronize()
        return {name: round(ms, 4) for name, (launches, ms) in p.profile_read(True).items()}

    if "min" in legs:
        for rep in range(args.repeat):
            print(json.dumps({"metric": "point_min_ms_per_step", **base, "repeat": rep, **timed(False, "binned")}), flush=True)
    if "stat" in legs:
        for path in [s for s in args.paths.split(",") if s]:
            out = {"metric": "cell_stats_ms_per_step", **base, "path": path}
            out.update(timed(True, path))
            out["kernels_ms"] = kernels(True, path)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
