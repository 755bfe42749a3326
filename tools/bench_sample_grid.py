#!/usr/bin/env python3
"""What sampling a band at the points costs (profiles/sample_grid.md), on C2's shape: 50 M uniform points
over a 4096 x 4096 surface, everything resident in HBM, device events on the stream, the median of 9 after 2 warm-up calls.

  kernel   pcr_hip_sample_grid, Nearest and Bilinear, value channel given, for the points in random order and sorted by row;
           ms and bytes/s at 28 B per point (x, y, value, output, one band cell)
  copy     pcr_hip_copy_kernel moving the same byte count (14 B read + 14 B written per point), non-temporal and plain
  host     the round trip the feature replaces: cloud to the host, pcr.sample_grid on the host cloud (OpenMP), channel back
  pass 2   ingest_async of a Device cloud into Max(hag | first returns) + Count(hag > 2) + Count, the channel derived at
           ingest against the same pipeline fed a cloud that already carries it, alternating; the bands must be equal

Prints one JSON line; SG_POINTS / SG_GRID shrink the shape, SG_OUT names a file that gets the JSON as well.

    python tools/bench_sample_grid.py"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
os.environ["PCR_REQUIRE_GPU_ENGINE"] = "1"
import pcr                                                        # noqa: E402
import pcr._cabi as A                                             # noqa: E402

L = A.lib()
N = int(os.environ.get("SG_POINTS", 50_000_000))
G = int(os.environ.get("SG_GRID", 4096))
REPS = 9
out = {"points": N, "surface": [G, G]}


def events():
    a, b = C.c_void_p(), C.c_void_p()
    A.check(L.pcr_hip_event_create(C.byref(a)))
    A.check(L.pcr_hip_event_create(C.byref(b)))
    return a, b


def timed(fn, stream=None, reps=REPS, warm=2):
    a, b = events()
    for _ in range(warm):
        fn()
    A.check(L.pcr_hip_stream_synchronize(stream))
    ms = []
    for _ in range(reps):
        A.check(L.pcr_hip_event_record(a, stream))
        fn()
        A.check(L.pcr_hip_event_record(b, stream))
        t = C.c_float(0)
        A.check(L.pcr_hip_event_elapsed_ms(a, b, C.byref(t)))
        ms.append(float(t.value))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


rng = np.random.default_rng(1)
x = rng.uniform(0.0, float(G), N)
y = rng.uniform(0.0, float(G), N)
z = rng.uniform(0.0, 60.0, N).astype(np.float32)
band = (rng.standard_normal((G, G)) * 5.0 + 20.0).astype(np.float32)
grid = A.make_grid((0.0, 0.0, float(G), float(G)), dims=(G, G), tile=(G, G))
d_band = A.DeviceBuffer.from_numpy(band)
d_out = A.DeviceBuffer(4 * N)
order = np.argsort((np.floor(float(G) - y)).astype(np.int32), kind="stable")

for label, idx in (("random", None), ("row_ordered", order)):
    dx = A.DeviceBuffer.from_numpy(x if idx is None else x[idx])
    dy = A.DeviceBuffer.from_numpy(y if idx is None else y[idx])
    dz = A.DeviceBuffer.from_numpy(z if idx is None else z[idx])
    for mode, mname in ((0, "nearest"), (1, "bilinear")):
        r = timed(lambda: A.check(L.pcr_hip_sample_grid(C.byref(grid), d_band.ptr, G, dx.ptr, dy.ptr, dz.ptr, N, mode, d_out.ptr, None)))
        r["GBps_at_28B_per_point"] = 28.0 * N / (r["median_ms"] * 1e6)
        out[f"kernel_{label}_{mname}"] = r
        print(label, mname, r, flush=True)
    dx.free(); dy.free(); dz.free()

# the copy kernel moving the same byte count: 14 B read + 14 B written per point
half = (14 * N) // 16 * 16
src, dst = A.DeviceBuffer(half), A.DeviceBuffer(half)
A.check(L.pcr_hip_memset(src.ptr, 1, half, None))
for nt in (1, 0):
    r = timed(lambda: A.check(L.pcr_hip_copy_kernel(dst.ptr, src.ptr, half, nt, None)))
    r["GBps"] = 2.0 * half / (r["median_ms"] * 1e6)
    out[f"copy_kernel_{'nontemporal' if nt else 'plain'}"] = r
    print("copy", nt, r, flush=True)
src.free(); dst.free(); d_out.free(); d_band.free()


# ---- pass 2: the channel derived at ingest against a cloud that already carries it ---------------------------------------------
def make_cfg(surface):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(G), float(G))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = pcr.ExecutionMode.GPU
    cfg.result_location = pcr.MemoryLocation.Device
    specs = []
    for t, ch, pred in ((pcr.ReductionType.Max, "hag", ("ret", pcr.CompareOp.Equal, 1.0)),
                        (pcr.ReductionType.Count, "z", ("hag", pcr.CompareOp.Greater, 2.0)), (pcr.ReductionType.Count, "z", None)):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = ch, t
        if pred:
            r.filter.add(*pred)
        specs.append(r)
    cfg.reductions = specs
    if surface:
        cfg.surface_channels = [pcr.SurfaceChannelConfig("hag", "z", pcr.SampleMode.Bilinear)]
    return cfg


def cloud_of(channels):
    c = pcr.PointCloud.create(N)
    c.set_x_array(x)
    c.set_y_array(y)
    for name, v in channels.items():
        c.add_channel(name, pcr.DataType.Float32)
        c.set_channel_array_f32(name, v)
    return c


ret = rng.integers(1, 3, N).astype(np.float32)
surf = pcr.Grid.create(G, G, [pcr.BandDesc()])
surf.set_band_array(0, band)
surf.set_geometry(make_cfg(False).grid)
host_cloud = cloud_of({"z": z, "ret": ret})

# the host round trip the feature replaces: cloud to the host, the host loop on the machine's threads, the channel back
dev_cloud = host_cloud.to_device()
t0 = time.perf_counter()
back = dev_cloud.to_host()
t1 = time.perf_counter()
pcr.sample_grid(back, surf, 0, "hag", "z")
t2 = time.perf_counter()
hag = np.array(back.channel_array_f32("hag"))
d_hag = A.DeviceBuffer.from_numpy(hag)
t3 = time.perf_counter()
out["host_round_trip"] = {"cloud_to_host_ms": 1e3 * (t1 - t0), "host_loop_ms": 1e3 * (t2 - t1), "channel_back_ms": 1e3 * (t3 - t2),
                          "total_ms": 1e3 * (t3 - t0), "omp_threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
print("host round trip", out["host_round_trip"], flush=True)
d_hag.free()
del back

pre_cloud = cloud_of({"z": z, "ret": ret, "hag": hag}).to_device()
derived = pcr.Pipeline.create(make_cfg(True))
precomputed = pcr.Pipeline.create(make_cfg(False))
assert derived is not None and precomputed is not None, pcr.pipeline_create_error()
derived.set_surface("hag", surf.to(pcr.MemoryLocation.Device))
res = {"derived": [], "precomputed": []}
for rep in range(7):                                             # alternating; the first two are warm-up
    for name, p, c in (("derived", derived, dev_cloud), ("precomputed", precomputed, pre_cloud)):
        a, b = events()
        s = C.c_void_p(p.stream_ptr())
        p.synchronize()
        A.check(L.pcr_hip_event_record(a, s))
        p.ingest_async(c)
        A.check(L.pcr_hip_event_record(b, s))
        t = C.c_float(0)
        A.check(L.pcr_hip_event_elapsed_ms(a, b, C.byref(t)))
        if rep >= 2:
            res[name].append(float(t.value))
for name in res:
    out[f"pass2_ingest_{name}"] = {"median_ms": float(np.median(res[name])), "min_ms": min(res[name]), "max_ms": max(res[name])}
derived.finalize()
precomputed.finalize()
same = all(np.array_equal(np.array(derived.result().to_host().band_array(b)).view(np.uint32),
                          np.array(precomputed.result().to_host().band_array(b)).view(np.uint32)) for b in range(3))
out["pass2_bands_equal"] = bool(same)
print("pass 2", {k: v for k, v in out.items() if k.startswith("pass2")}, flush=True)

if os.environ.get("SG_OUT"):
    with open(os.environ["SG_OUT"], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
