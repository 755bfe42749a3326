"""LAS input on the GPU: the decode kernel (pcr_hip_las_decode) against its host twin bit for bit, read_las into HBM, and
Pipeline.ingest_file of a `.las` on the HIP engine -- raw records over PCIe, decoded in HBM -- against ingest of the model
cloud (tests/las_common.py).  Every bad argument is rejected on the host: nothing here can fault."""
import ctypes as C

import numpy as np
import pytest

import las_common as LC
import pcr
from conftest import load_cabi
from test_las_io import ORIGIN, assert_same_bands, bands, model_cloud, spec

pytestmark = pytest.mark.gpu

A = load_cabi()
RUN = 256 * A.LAS_RECORDS_PER_LANE             # records a workgroup owns
COUNTS = [1, 63, 64, 255, 256, 257, 1000, 4 * RUN + 3]
# record length -> a point format that allows it.  20-70: a record start at every residue mod 16 and records across the
# 16-byte staging boundary; 126 / 127: the longest record staged through LDS and the first read straight from memory; 200
LENGTHS = {20: 0, 21: 0, 26: 2, 28: 1, 29: 1, 30: 6, 34: 3, 36: 7, 38: 8, 41: 8, 67: 10, 70: 10, 126: 3, 127: 7, 200: 5}
SENTINEL = -7.0


def decode_both(fmt, rec, n, wanted, scale, offset):
    """(device outputs, host outputs) for the first n records; arrays have n + 1 elements, the last one a sentinel."""
    L = A.lib()
    length = rec.dtype.itemsize
    lay = A.LasLayout(fmt, length, (C.c_double * 3)(*scale), (C.c_double * 3)(*offset), ORIGIN)
    raw = np.zeros(n * length + 16, dtype=np.uint8)                # the 16 bytes of slack the kernel's staging may read
    raw[:n * length] = np.frombuffer(rec[:n].tobytes(), dtype=np.uint8)
    host = {"x": np.full(n + 1, SENTINEL), "y": np.full(n + 1, SENTINEL)}
    for name in wanted:
        host[name] = np.full(n + 1, SENTINEL, dtype=np.float32)
    hp = (C.c_void_p * len(A.LAS_CHANNELS))()
    for name in wanted:
        hp[A.LAS_CHANNELS.index(name)] = host[name].ctypes.data
    A.check(L.pcr_hip_las_decode_host(C.byref(lay), raw.ctypes.data, n, host["x"].ctypes.data, host["y"].ctypes.data, hp, 1))
    d_raw = A.DeviceBuffer.from_numpy(raw)
    dev = {k: A.DeviceBuffer.from_numpy(np.full(n + 1, SENTINEL, dtype=v.dtype)) for k, v in host.items()}
    dp = (C.c_void_p * len(A.LAS_CHANNELS))()
    for name in wanted:
        dp[A.LAS_CHANNELS.index(name)] = dev[name].ptr.value
    A.check(L.pcr_hip_las_decode(C.byref(lay), d_raw.ptr, n, dev["x"].ptr, dev["y"].ptr, dp, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = {k: b.to_numpy() for k, b in dev.items()}
    for b in list(dev.values()) + [d_raw]:
        b.free()
    return got, host


@pytest.mark.parametrize("length", sorted(LENGTHS))
def test_kernel_equals_host_decoder(length):
    fmt = LENGTHS[length]
    nmax = max(COUNTS)
    fields = LC.make_fields(fmt, nmax, np.random.default_rng(length))
    rec = LC.pack_records(fmt, fields, length - LC.MIN_LENGTH[fmt])
    assert rec.dtype.itemsize == length
    scale, offset = (0.001, 1e-7, 0.01), (4.5e6, 0.0, 100.0)
    model = LC.expected(fmt, fields, scale, offset, ORIGIN)
    every = LC.channels_of(fmt)
    for n in COUNTS:
        for wanted in (every, ["z"], []):
            got, host = decode_both(fmt, rec, n, wanted, scale, offset)
            for k in got:
                assert got[k][n] == SENTINEL and host[k][n] == SENTINEL, f"length {length} n {n} {k}: wrote past the end"
            LC.assert_bits_equal({k: v[:n] for k, v in got.items()}, {k: v[:n] for k, v in host.items()},
                                 f"length {length} n {n} channels {len(wanted)}")
            LC.assert_bits_equal({k: v[:n] for k, v in got.items()}, {k: model[k][:n] for k in got},
                                 f"model: length {length} n {n} channels {len(wanted)}")


def test_misaligned_records_are_refused_on_the_host():
    L = A.lib()
    lay = A.LasLayout(1, 28, (C.c_double * 3)(1, 1, 1), (C.c_double * 3)(0, 0, 0), 0.0)
    buf = A.DeviceBuffer(28 * 4 + 32)
    out = A.DeviceBuffer(64)
    assert L.pcr_hip_las_decode(C.byref(lay), buf.ptr.value + 4, 4, out.ptr, out.ptr, None, None) == 1
    assert b"16-byte aligned" in L.pcr_hip_last_error()


@pytest.mark.parametrize("fmt,extra", [(1, 0), (8, 5)])
def test_read_las_into_device_memory_equals_host_read(tmp_path, fmt, extra):
    n = 3000
    fields = LC.make_fields(fmt, n, np.random.default_rng(fmt))
    rec = LC.pack_records(fmt, fields, extra)
    scale, offset = (0.01, 0.01, 0.001), (4.5e6, 0.0, 0.0)
    path = str(tmp_path / "t.las")
    LC.write_las(path, fmt, rec, scale, offset, version=(1, 4), epsg=32633)
    names = LC.channels_of(fmt)
    host = pcr.read_las(path, gps_time_origin=ORIGIN)
    dev = pcr.read_las(path, gps_time_origin=ORIGIN, location=pcr.MemoryLocation.Device)
    assert dev.location() == pcr.MemoryLocation.Device and dev.count() == n and dev.crs().epsg == 32633
    want = LC.expected(fmt, fields, scale, offset, ORIGIN)
    LC.assert_bits_equal(LC.cloud_arrays(host, names), want, "host")
    LC.assert_bits_equal(LC.cloud_arrays(dev.to_host(), names), want, "device")
    pinned = pcr.read_point_cloud(path, location=pcr.MemoryLocation.HostPinned)
    LC.assert_bits_equal(LC.cloud_arrays(pinned, names), LC.expected(fmt, fields, scale, offset, 0.0), "pinned")
    sub = pcr.read_las(path, channels=["intensity"], location=pcr.MemoryLocation.Device)
    assert sub.channel_names() == ["intensity"]
    LC.assert_bits_equal(LC.cloud_arrays(sub.to_host(), ["intensity"]), {k: want[k] for k in ("x", "y", "intensity")}, "subset")


# ---- Pipeline.ingest_file on the HIP engine ---------------------------------------------------------------------------------------
W, H, NPTS = 64, 48, 5000
T = pcr.ReductionType
GPS0 = 3.2e8


def grid_fields(fmt, lonlat=False):
    """NPTS points inside the grid.  z is a multiple of 1/8 and intensity an integer, so that Sum and Average do not depend
    on the order in which a cell's points are added."""
    rng = np.random.default_rng(9)
    f = LC.make_fields(fmt, NPTS, rng)
    if lonlat:                                   # around 15 E 45 N, scale 1e-7 degrees: ~55 m x ~39 m
        f["X"] = (150_000_000 + rng.integers(100, 7000, NPTS)).astype(np.int32)
        f["Y"] = (450_000_000 + rng.integers(100, 3500, NPTS)).astype(np.int32)
    else:
        f["X"] = rng.integers(1000, (W - 1) * 1000, NPTS).astype(np.int32)
        f["Y"] = rng.integers(1000, (H - 1) * 1000, NPTS).astype(np.int32)
    f["Z"] = rng.integers(-400, 8000, NPTS).astype(np.int32)
    f["intensity"] = rng.integers(0, 4096, NPTS).astype(np.uint16)
    if fmt <= 5:
        f["b15"] = (np.arange(NPTS) % 5).astype(np.uint8)
    else:
        f["classification"] = (np.arange(NPTS) % 5).astype(np.uint8)
    f["gps_time"] = GPS0 + rng.uniform(0.0, 5000.0, NPTS)
    return f


REDUCTIONS = [("intensity", T.Sum, ""), ("z", T.Max, ""), ("z", T.Min, ""), ("z", T.Count, ""), ("z", T.MostRecent, "gps_time"),
              ("z", T.Average, "")]
NAMES = ["z", "intensity", "gps_time"]


def gpu_config(bounds=(0.0, 0.0, float(W), float(H)), filter_class=None, crs=None, reductions=REDUCTIONS):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(*bounds)
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = (bounds[2] - bounds[0]) / W, -(bounds[3] - bounds[1]) / H
    cfg.grid.compute_dimensions()
    assert (cfg.grid.width, cfg.grid.height) == (W, H)
    if crs is not None:
        cfg.grid.crs = crs
    cfg.exec_mode = pcr.ExecutionMode.GPU
    cfg.reductions = [spec(c, t, ts) for c, t, ts in reductions]
    cfg.las_gps_time_origin = GPS0
    if filter_class is not None:
        f = pcr.FilterSpec()
        f.add("classification", pcr.CompareOp.Equal, float(filter_class))
        cfg.filter = f
    return cfg


def create(cfg):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == "hip"
    return p


def check_file_against_model(path, cfg_of, want, names, chunk, prepare=lambda c: c):
    a = create(cfg_of())
    assert a.ingest_file(path, chunk) == NPTS
    whole = create(cfg_of())
    whole.ingest(prepare(model_cloud(want, names)))
    chunked = create(cfg_of())
    for lo in range(0, NPTS, chunk):
        chunked.ingest(prepare(model_cloud(want, names, lo, min(lo + chunk, NPTS))))
    got, one, parts = bands(a), bands(whole), bands(chunked)
    assert_same_bands(got[:5], one[:5], f"chunk {chunk}: Sum / Max / Min / Count / MostRecent against one ingest")
    assert_same_bands(got[5:], parts[5:], f"chunk {chunk}: Average against the same chunks")
    assert np.isfinite(got[3]).sum() > W * H // 4              # (the points did land in the grid)


@pytest.mark.parametrize("chunk", [1000, 4096, 10000])
def test_ingest_file_las_on_the_hip_engine(tmp_path, chunk):
    fmt = 3
    f = grid_fields(fmt)
    scale, offset = (0.001, 0.001, 0.125), (0.0, 0.0, 0.0)
    path = str(tmp_path / "grid.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f, 2), scale, offset)
    want = LC.expected(fmt, f, scale, offset, GPS0)
    check_file_against_model(path, gpu_config, want, NAMES, chunk)


def test_ingest_file_las_with_a_classification_filter(tmp_path):
    fmt = 6
    f = grid_fields(fmt)
    scale, offset = (0.001, 0.001, 0.125), (0.0, 0.0, 0.0)
    path = str(tmp_path / "grid.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset, version=(1, 4))
    want = LC.expected(fmt, f, scale, offset, GPS0)
    a = create(gpu_config(filter_class=2))
    assert a.ingest_file(path, 2048) == NPTS
    assert a.stats().points_processed == NPTS // 5
    b = create(gpu_config(filter_class=2))
    for lo in range(0, NPTS, 2048):
        b.ingest(model_cloud(want, NAMES + ["classification"], lo, min(lo + 2048, NPTS)))
    assert_same_bands(bands(a), bands(b), "filter")


def test_ingest_file_las_reprojects_from_its_geokey_crs(tmp_path):
    fmt = 1
    f = grid_fields(fmt, lonlat=True)
    scale, offset = (1e-7, 1e-7, 0.125), (0.0, 0.0, 0.0)
    path = str(tmp_path / "lonlat.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset, epsg=4326, geographic=True)
    want = LC.expected(fmt, f, scale, offset, GPS0)
    utm = pcr.CRS.from_epsg(32633)
    ux, uy = pcr.transform_xy(4326, 32633, want["x"], want["y"])
    x0, y0 = np.floor(ux.min()) - 1.0, np.floor(uy.min()) - 1.0
    bounds = (x0, y0, x0 + W, y0 + H)                          # 1 m cells
    assert ux.max() < bounds[2] and uy.max() < bounds[3]

    def tagged(c):
        c.set_crs(pcr.CRS.from_epsg(4326))
        d = c.to_device()
        pcr.reproject(d, utm)                                  # the kernel ingest itself uses
        return d

    check_file_against_model(path, lambda: gpu_config(bounds, crs=utm), want, NAMES, 2048, prepare=tagged)


def test_a_channel_the_format_lacks_is_named(tmp_path):
    fmt = 1
    path = str(tmp_path / "grid.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, grid_fields(fmt)), (0.001, 0.001, 0.125), (0.0, 0.0, 0.0))
    p = create(gpu_config(reductions=[("z", T.Max, ""), ("red", T.Max, "")]))
    with pytest.raises(RuntimeError, match="point format 1 has no channel 'red'"):
        p.ingest_file(path, 1000)
