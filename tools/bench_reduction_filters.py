#!/usr/bin/env python3
"""What per-reduction filters (ReductionSpec.filter) cost and save, on C2's shape (50 M uniform points, 4096 x 4096).  Prints one
JSON line per leg.

  sweep    pcr_hip_filter_classes, four classes over two shared channels, against four pcr_hip_filter_mask calls on the same
           inputs (C-ABI, device arrays): ms, achieved bytes/s (the sweep moves 2 x 4 B in and 4 x 1 B out per point), ratio
  ingest   one ingest + finalize of four Point groups (Min, Max, Sum, Count of four channels), each with a filter of its own,
           device-resident cloud -- and with --unfiltered the same four groups without filters (runs on a tree without the
           feature: the yardstick of what losing the fused finalize costs)
  host     the same four filtered specs on a HOST-resident (pageable) cloud in ONE pipeline, against four pipelines with one
           PipelineConfig.filter each: the file read / PCIe argument, measured once

Timing as in bench.py: fresh pipelines created before the clock starts, W untimed warm-up steps, K timed steps each between
two device synchronisations, the MEDIAN of the K.

    python tools/bench_reduction_filters.py [--legs sweep,ingest,host] [--unfiltered] [--steps 10] [--warmup 3]
                                            [--points 50000000] [--grid 4096]"""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pcr  # noqa: E402
from pcr import _cabi as A  # noqa: E402

VALUES = ("z", "intensity", "u", "w")
# (type, value channel, its filter): DTM, DSM, intensity of single returns, density of a class
SPECS = (("Min", "z", (("cls", "Equal", 2.0),)), ("Max", "z2", (("ret", "Equal", 1.0),)),
         ("Sum", "intensity", (("ret", "Equal", 1.0), ("cls", "NotEqual", 7.0))), ("Count", "u", (("cls", "Equal", 5.0),)))
CHANNELS = ("z", "z2", "intensity", "u", "cls", "ret")


def fill(c, n, G, where):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    cols = {"x": torch.empty(n, dtype=torch.float64, device="cuda").uniform_(2.0, G - 2.0, generator=gen),
            "y": torch.empty(n, dtype=torch.float64, device="cuda").uniform_(2.0, G - 2.0, generator=gen)}
    for name in CHANNELS:
        if name == "cls":
            cols[name] = torch.randint(1, 8, (n,), generator=gen, device="cuda").to(torch.float32)
        elif name == "ret":
            cols[name] = torch.randint(1, 4, (n,), generator=gen, device="cuda").to(torch.float32)
        else:
            cols[name] = torch.empty(n, dtype=torch.float32, device="cuda").uniform_(0.0, 1.0, generator=gen)
    if where == "device":
        ptrs = c.device_ptrs()
        for name, t in cols.items():
            dst = torch.as_tensor(pcr.DeviceArrayView(ptrs[name], (n,), "<f8" if name in "xy" else "<f4", owner=c), device="cuda")
            dst.copy_(t)
    else:
        c.set_x_array(cols["x"].cpu().numpy())
        c.set_y_array(cols["y"].cpu().numpy())
        for name in CHANNELS:
            c.set_channel_array_f32(name, cols[name].cpu().numpy())
    torch.cuda.synchronize()


def make_cloud(n, G, where):
    c = pcr.PointCloud.create(n, pcr.MemoryLocation.Device) if where == "device" else pcr.PointCloud.create(n)
    if c is None:
        raise MemoryError("cannot allocate the cloud")
    for name in CHANNELS:
        c.add_channel(name, pcr.DataType.Float32)
    c.resize(n)
    fill(c, n, G, where)
    return c


def make_pipe(G, n, specs, filtered, cfg_filter=()):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(G), float(G))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = pcr.ExecutionMode.GPU
    reds = []
    for rtype, ch, preds in specs:
        r = pcr.ReductionSpec()
        r.value_channel, r.type = ch, getattr(pcr.ReductionType, rtype)
        if filtered:
            for name, op, v in preds:
                r.filter.add(name, getattr(pcr.CompareOp, op), v)
        reds.append(r)
    cfg.reductions = reds
    f = pcr.FilterSpec()
    for name, op, v in cfg_filter:
        f.add(name, getattr(pcr.CompareOp, op), v)
    cfg.filter = f
    cfg.result_location = pcr.MemoryLocation.Device
    cfg.gpu_pool_size_bytes = 24 * n + (64 << 20)
    p = pcr.Pipeline.create(cfg)
    if p is None:
        raise RuntimeError(pcr.pipeline_create_error())
    return p


def timed(make, step, warm, steps):
    """make() -> a fresh object per step, created before the clock starts; the median of `steps` timed steps in ms."""
    objs = [make() for _ in range(warm + steps)]
    for o in objs[:warm]:
        step(o)
    torch.cuda.synchronize()
    ms = []
    for o in objs[warm:]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(o)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]


def leg_sweep(args, out):
    n, L = args.points, A.lib()
    cloud = make_cloud(n, args.grid, "device")
    ptrs = cloud.device_ptrs()
    table = (("cls", 0, 2.0), ("ret", 0, 1.0), ("cls", 1, 7.0), ("cls", 0, 5.0))
    words = (0b0001, 0b0010, 0b0110, 0b1000)                    # SPECS' four filters
    preds = (A.Predicate * 4)()
    for k, (ch, op, v) in enumerate(table):
        preds[k].d_channel, preds[k].op, preds[k].value = ptrs[ch], op, v
    stride = (n + 15) // 16 * 16
    masks = A.DeviceBuffer(4 * stride)
    cw = (C.c_uint32 * 4)(*words)

    def sweep(_):
        A.check(L.pcr_hip_filter_classes(preds, 4, cw, 4, n, masks.ptr, stride, None, None))

    def four_calls(_):
        for j, w in enumerate(words):
            mine = [preds[k] for k in range(4) if w >> k & 1]
            A.check(L.pcr_hip_filter_mask((A.Predicate * len(mine))(*mine), len(mine), n, masks.ptr.value + j * stride, None, None))

    out["sweep_ms"], out["sweep_ms_min_max"] = timed(lambda: None, sweep, args.warmup, args.steps)
    out["four_calls_ms"], out["four_calls_ms_min_max"] = timed(lambda: None, four_calls, args.warmup, args.steps)
    out["sweep_bytes_per_point"] = 2 * 4 + 4 * 1
    out["sweep_TB_per_s"] = round(n * 12 / (out["sweep_ms"] * 1e-3) / 1e12, 3)
    out["four_calls_bytes_per_point"] = 5 * 4 + 4 * 1            # one channel per predicate of each call, one mask each
    out["four_calls_TB_per_s"] = round(n * 24 / (out["four_calls_ms"] * 1e-3) / 1e12, 3)
    out["four_calls_over_sweep"] = round(out["four_calls_ms"] / out["sweep_ms"], 3)


def leg_ingest(args, out):
    n, G = args.points, args.grid
    cloud = make_cloud(n, G, "device")

    def step(p):
        p.ingest(cloud)
        p.finalize()

    name = "unfiltered" if args.unfiltered else "filtered"
    out[name + "_ms"], out[name + "_ms_min_max"] = timed(lambda: make_pipe(G, n, SPECS, not args.unfiltered), step, args.warmup, args.steps)


def leg_host(args, out):
    n, G = args.points, args.grid
    cloud = make_cloud(n, G, "host")

    def one(p):
        p.ingest(cloud)
        p.finalize()

    def four(ps):
        for p in ps:
            p.ingest(cloud)
            p.finalize()

    out["one_pipeline_ms"], out["one_pipeline_ms_min_max"] = timed(lambda: make_pipe(G, n, SPECS, True), one, 1, args.host_steps)
    out["four_pipelines_ms"], out["four_pipelines_ms_min_max"] = timed(
        lambda: [make_pipe(G, n, [(t, ch, ())], False, preds) for t, ch, preds in SPECS], four, 1, args.host_steps)
    out["four_over_one"] = round(out["four_pipelines_ms"] / out["one_pipeline_ms"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="sweep,ingest,host")
    ap.add_argument("--unfiltered", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--grid", type=int, default=4096)
    args = ap.parse_args()
    for leg in [s for s in args.legs.split(",") if s]:
        out = {"metric": "reduction_filters_" + leg, "points": args.points, "grid": [args.grid, args.grid], "steps": args.steps,
               "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
        {"sweep": leg_sweep, "ingest": leg_ingest, "host": leg_host}[leg](args, out)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
