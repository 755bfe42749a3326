#!/usr/bin/env python3
"""What LAS input costs (profiles/las_ingest.md).  Prints JSON lines; --out also writes the whole result as a JSON file.

1. pcr_hip_las_decode alone: N format-1 (28 B) and format-7 (36 B) records in HBM, all channels wanted and `z` only, each next
   to pcr_hip_copy_kernel (non-temporal) moving the same number of bytes (records read + arrays written).  Every call between
   two device events: 2 warm-ups, then the median (min, max) of 10.  The decoded x of the last million records is compared
   with the NumPy model.
2. Pipeline.ingest_file end to end, from the page cache: the same N points as a format-1 `.las` (`z` + `intensity` wanted) and
   as the `.pcrp` that holds x, y and those two channels; Average(z) + Max(intensity) on a 4096 x 4096 grid; the two files
   alternate, the first round is a warm-up, three timed rounds each.  Host clock around ingest_file + synchronize().

    python tools/las_ingest_time.py [--points 50000000] [--out result.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pointcloud-raster_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ["PCR_REQUIRE_GPU_ENGINE"] = "1"
import las_common as LC  # noqa: E402
import pcr  # noqa: E402
from pcr import _cabi as A  # noqa: E402

L = A.lib()
ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=50_000_000)
ap.add_argument("--out", default="")
args = ap.parse_args()
N = args.points // 1_000_000 * 1_000_000
assert N > 0, "--points: at least one million"
PIECE = 1_000_000
out = {"n": N}


def event():
    e = C.c_void_p()
    A.check(L.pcr_hip_event_create(C.byref(e)))
    return e


def timed(fn, reps=10, warm=2):
    e0, e1 = event(), event()
    ms = []
    for k in range(warm + reps):
        A.check(L.pcr_hip_event_record(e0, None))
        fn()
        A.check(L.pcr_hip_event_record(e1, None))
        t = C.c_float(0)
        A.check(L.pcr_hip_event_elapsed_ms(e0, e1, C.byref(t)))
        if k >= warm:
            ms.append(t.value)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def kernel_numbers(fmt):
    rng = np.random.default_rng(fmt)
    rec = LC.pack_records(fmt, LC.make_fields(fmt, PIECE, rng))
    length = rec.dtype.itemsize
    piece = A.DeviceBuffer.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8))
    d_rec = A.DeviceBuffer(N * length + 16)
    for k in range(N // PIECE):
        A.check(L.pcr_hip_memcpy_d2d(d_rec.ptr.value + k * PIECE * length, piece.ptr, PIECE * length, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    names = LC.channels_of(fmt)
    dx, dy = A.DeviceBuffer(N * 8), A.DeviceBuffer(N * 8)
    chans = {name: A.DeviceBuffer(N * 4) for name in names}
    lay = A.LasLayout(fmt, length, (C.c_double * 3)(0.001, 0.001, 0.001), (C.c_double * 3)(0, 0, 0), 3.2e8)
    res = {}
    for label, wanted in (("all", names), ("z", ["z"])):
        ptrs = (C.c_void_p * len(A.LAS_CHANNELS))()
        for name in wanted:
            ptrs[A.LAS_CHANNELS.index(name)] = chans[name].ptr.value
        dec = timed(lambda: A.check(L.pcr_hip_las_decode(C.byref(lay), d_rec.ptr, N, dx.ptr, dy.ptr, ptrs, None)))
        traffic = N * (length + 16 + 4 * len(wanted))
        half = (traffic // 2) // 16 * 16
        src, dst = A.DeviceBuffer(half), A.DeviceBuffer(half)
        cp = timed(lambda: A.check(L.pcr_hip_copy_kernel(dst.ptr, src.ptr, half, 1, None)))
        src.free(); dst.free()
        res[label] = {"record_length": length, "channels": len(wanted), "bytes_moved": traffic, "decode_ms": dec, "copy_ms": cp,
                      "decode_GBps": traffic / dec[0] / 1e6, "copy_GBps": 2 * half / cp[0] / 1e6, "ratio_decode_over_copy": dec[0] / cp[0],
                      "Gpts_per_s": N / dec[0] / 1e6}
        print(fmt, label, json.dumps(res[label]), flush=True)
    # spot check of what was timed: first piece against the model
    want = LC.expected(fmt, LC.make_fields(fmt, PIECE, np.random.default_rng(fmt)), (0.001,) * 3, (0, 0, 0), 3.2e8)
    got_x = np.empty(PIECE)
    A.check(L.pcr_hip_memcpy_d2h(got_x.ctypes.data, dx.ptr.value + (N - PIECE) * 8, PIECE * 8, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    assert np.array_equal(got_x, want["x"])
    for b in [piece, d_rec, dx, dy] + list(chans.values()):
        b.free()
    return res


out["kernel_format_1"] = kernel_numbers(1)
out["kernel_format_7"] = kernel_numbers(7)

# ---- ingest_file end to end, from the page cache -------------------------------------------------------------------------------
W = H = 4096
tmp = tempfile.mkdtemp(prefix="las_measure_")
rng = np.random.default_rng(1)
fields = LC.make_fields(1, N, rng)
fields["X"] = rng.integers(1000, (W - 1) * 1000, N).astype(np.int32)
fields["Y"] = rng.integers(1000, (H - 1) * 1000, N).astype(np.int32)
fields["Z"] = rng.integers(0, 500_000, N).astype(np.int32)
scale, offset = (0.001, 0.001, 0.001), (0.0, 0.0, 0.0)
las_path, pcrp_path = os.path.join(tmp, "t.las"), os.path.join(tmp, "t.pcrp")
LC.write_las(las_path, 1, LC.pack_records(1, fields), scale, offset)
want = LC.expected(1, fields, scale, offset)
cloud = pcr.PointCloud.create(N)
cloud.resize(N)
cloud.set_x_array(want["x"]); cloud.set_y_array(want["y"])
for name in ("z", "intensity"):
    cloud.add_channel(name, pcr.DataType.Float32)
    cloud.set_channel_array_f32(name, want[name])
pcr.write_point_cloud(pcrp_path, cloud)
del cloud, fields
print("files", os.path.getsize(las_path), os.path.getsize(pcrp_path), flush=True)


def pipeline():
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = pcr.ExecutionMode.GPU
    specs = []
    for ch, t in (("z", pcr.ReductionType.Average), ("intensity", pcr.ReductionType.Max)):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = ch, t
        specs.append(r)
    cfg.reductions = specs
    p = pcr.Pipeline.create(cfg)
    assert p is not None and p.engine() == "hip"
    return p


times = {"las": [], "pcrp": []}
results = {}
for rep in range(4):                       # alternating; the first round warms the page cache and the code objects
    for kind, path in (("las", las_path), ("pcrp", pcrp_path)):
        p = pipeline()
        t0 = time.perf_counter()
        n = p.ingest_file(path)
        p.synchronize()
        dt = time.perf_counter() - t0
        assert n == N
        if rep:
            times[kind].append(dt)
        if rep == 3:
            p.finalize()
            results[kind] = [np.array(p.result().band_array(b)) for b in range(2)]
        del p
mx_equal = bool(np.array_equal(results["las"][1], results["pcrp"][1], equal_nan=True))
avg_close = bool(np.allclose(results["las"][0], results["pcrp"][0], rtol=1e-5, equal_nan=True))
out["ingest_file"] = {k: {"seconds": v, "median_Mpts_per_s": N / float(np.median(v)) / 1e6} for k, v in times.items()}
out["ingest_file"]["max_band_equal"] = mx_equal
out["ingest_file"]["average_band_close"] = avg_close
os.remove(las_path); os.remove(pcrp_path); os.rmdir(tmp)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out["ingest_file"]))
