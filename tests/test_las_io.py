"""LAS input on the CPU: the header parser, the host decoder (pcr_hip_las_decode_host, the same header the gfx950 kernel is
built from), read_point_cloud / read_las / PointCloudReader and ExecutionMode.CPU's ingest_file, all against the ASPRS layout
restated in NumPy (tests/las_common.py).  Every coordinate and channel is compared bit for bit."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import las_common as LC
import pcr
from conftest import ROOT, load_cabi

PKG = os.path.join(ROOT, "pointcloud-raster_amd")
N = 600                                        # > 256: every value of the packed bytes occurs
ORIGIN = 3.2e8 + 123.5
# (scale, offset) mixes: 0.01 / 0.001 / 1e-7 and offsets 0 / 4.5e6
GEOM = [((0.01, 0.01, 0.01), (0.0, 0.0, 0.0)), ((0.001, 0.001, 0.001), (4.5e6, 4.5e6, 0.0)),
        ((1e-7, 1e-7, 0.01), (0.0, 4.5e6, 100.0))]
FORMATS = [0, 1, 2, 3, 6, 7, 8, 5, 10]         # 5 and 10: wave-packet bytes behind the attributes


def make_file(tmp_path, fmt, geom=0, extra=0, n=N, name=None, **kw):
    rng = np.random.default_rng(100 + fmt)
    fields = LC.make_fields(fmt, n, rng)
    rec = LC.pack_records(fmt, fields, extra)
    scale, offset = GEOM[geom]
    path = str(tmp_path / (name or f"f{fmt}.las"))
    LC.write_las(path, fmt, rec, scale, offset, **kw)
    return path, fields, rec, scale, offset


@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip_every_format(tmp_path, fmt):
    geom = fmt % 3
    path, fields, rec, scale, offset = make_file(tmp_path, fmt, geom, extra=(3 if fmt in (1, 7) else 0),
                                                 version=(1, 4) if fmt >= 6 else (1, 2))
    names = LC.channels_of(fmt)
    want = LC.expected(fmt, fields, scale, offset, 0.0)
    cloud = pcr.read_point_cloud(path)
    assert cloud.count() == N and sorted(cloud.channel_names()) == sorted(names)
    LC.assert_bits_equal(LC.cloud_arrays(cloud, names), want, f"read_point_cloud fmt {fmt}")
    # read_las with an origin and a subset
    sub = ["z", "classification"] + (["gps_time"] if fmt in LC.HAS_GPS else [])
    cloud = pcr.read_las(path, channels=sub, gps_time_origin=ORIGIN)
    want_o = LC.expected(fmt, fields, scale, offset, ORIGIN)
    assert sorted(cloud.channel_names()) == sorted(sub)
    LC.assert_bits_equal(LC.cloud_arrays(cloud, sub), {k: want_o[k] for k in ["x", "y"] + sub}, f"read_las fmt {fmt}")
    if fmt in LC.HAS_GPS:                      # the origin is what keeps sub-second resolution in Float32
        t = np.array(cloud.channel_array_f32("gps_time"), dtype=np.float64)
        assert np.abs(t[4:] - (fields["gps_time"][4:] - ORIGIN)).max() < 1e-3


@pytest.mark.parametrize("chunk", [1, 7, N + 1])
def test_reader_chunks_rewind_eof(tmp_path, chunk):
    fmt = 3
    n = 40 if chunk == 1 else N
    path, fields, rec, scale, offset = make_file(tmp_path, fmt, 1, n=n)
    names = LC.channels_of(fmt)
    want = LC.expected(fmt, fields, scale, offset, ORIGIN)
    r = pcr.PointCloudReader.open(path, gps_time_origin=ORIGIN)
    assert r.format() == pcr.PointCloudFormat.LAS and r.info().num_points == n and not r.eof()
    for attempt in range(2):
        got = {k: [] for k in ["x", "y"] + names}
        buf = pcr.PointCloud.create(chunk)
        while True:
            k = r.read_chunk(buf, chunk)
            if k == 0:
                break
            assert k == buf.count() <= chunk
            for key, a in LC.cloud_arrays(buf, names).items():
                got[key].append(a.copy())
        assert r.eof()
        LC.assert_bits_equal({k: np.concatenate(v) for k, v in got.items()}, want, f"chunk {chunk} pass {attempt}")
        r.rewind()
        assert not r.eof()
    r = pcr.PointCloudReader.open(path, channels=["intensity"])
    buf = pcr.PointCloud.create(n)
    assert r.read_chunk(buf, n) == n and buf.channel_names() == ["intensity"]


@pytest.mark.parametrize("fmt,extra", [(1, 0), (2, 1), (6, 0), (8, 3)])
def test_host_decoder_through_ctypes(fmt, extra):
    A = load_cabi()
    L = A.lib()
    n = 20_000                                  # several 4 K-record parts: four threads really run
    fields = LC.make_fields(fmt, n, np.random.default_rng(fmt))
    rec = LC.pack_records(fmt, fields, extra)
    scale, offset = GEOM[1]
    want = LC.expected(fmt, fields, scale, offset, ORIGIN)
    lay = A.LasLayout(fmt, rec.dtype.itemsize, (C.c_double * 3)(*scale), (C.c_double * 3)(*offset), ORIGIN)
    raw = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    for threads in (1, 4):
        out = {"x": np.full(n + 1, -7.0), "y": np.full(n + 1, -7.0)}
        ptrs = (C.c_void_p * len(A.LAS_CHANNELS))()
        for c, name in enumerate(A.LAS_CHANNELS):
            if name in want:
                out[name] = np.full(n + 1, -7.0, dtype=np.float32)
                ptrs[c] = out[name].ctypes.data
        assert L.pcr_hip_las_decode_host(C.byref(lay), raw.ctypes.data, n, out["x"].ctypes.data, out["y"].ctypes.data,
                                         ptrs, threads) == 0, L.pcr_hip_last_error()
        assert all(a[n] == -7.0 for a in out.values())
        LC.assert_bits_equal({k: a[:n] for k, a in out.items()}, want, f"fmt {fmt} threads {threads}")


def test_decode_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    x = np.zeros(4)
    rec = np.zeros(4 * 40, dtype=np.uint8)
    ptrs = (C.c_void_p * len(A.LAS_CHANNELS))()

    def lay(fmt, length):
        return A.LasLayout(fmt, length, (C.c_double * 3)(1, 1, 1), (C.c_double * 3)(0, 0, 0), 0.0)

    for fn, tail in ((L.pcr_hip_las_decode, None), (L.pcr_hip_las_decode_host, 1)):
        call = lambda layout, r, n, px, py, ch: fn(layout, r, n, px, py, ch, tail)  # noqa: E731
        assert call(None, rec.ctypes.data, 4, x.ctypes.data, x.ctypes.data, ptrs) == 1
        assert b"null layout" in L.pcr_hip_last_error()
        assert call(C.byref(lay(11, 40)), rec.ctypes.data, 4, x.ctypes.data, x.ctypes.data, ptrs) == 1
        assert b"point format 11" in L.pcr_hip_last_error()
        assert call(C.byref(lay(1, 27)), rec.ctypes.data, 4, x.ctypes.data, x.ctypes.data, ptrs) == 1
        assert b"record_length 27" in L.pcr_hip_last_error()
        assert call(C.byref(lay(1, 28)), rec.ctypes.data, 4, None, x.ctypes.data, ptrs) == 1
        assert b"null x or y" in L.pcr_hip_last_error()
        red = (C.c_void_p * len(A.LAS_CHANNELS))()
        red[A.LAS_CHANNELS.index("red")] = x.ctypes.data
        assert call(C.byref(lay(1, 28)), rec.ctypes.data, 4, x.ctypes.data, x.ctypes.data, red) == 1
        assert b"does not have it" in L.pcr_hip_last_error()
        assert call(C.byref(lay(1, 28)), None, 0, None, None, None) == 0          # n == 0: nothing to do, nothing launched


def test_info_counts_channels_bounds_crs(tmp_path):
    path, fields, rec, scale, offset = make_file(tmp_path, 3, 1, epsg=32633)
    info = pcr.read_point_cloud_info(path)
    want = LC.expected(3, fields, scale, offset)
    assert info.num_points == N
    assert [c.name for c in info.channels] == LC.channels_of(3)
    assert all(c.dtype == pcr.DataType.Float32 for c in info.channels)
    b = info.bounds
    assert (b.min_x, b.min_y, b.max_x, b.max_y) == (want["x"].min(), want["y"].min(), want["x"].max(), want["y"].max())
    assert info.crs.epsg == 32633 and pcr.read_point_cloud(path).crs().epsg == 32633
    path, *_ = make_file(tmp_path, 1, 0, epsg=4326, geographic=True, name="geo.las")
    assert pcr.read_point_cloud_info(path).crs.epsg == 4326
    wkt = 'PROJCS["WGS 84 / UTM zone 33N",GEOGCS["WGS 84"],AUTHORITY["EPSG","32633"]]'
    path, *_ = make_file(tmp_path, 6, 0, version=(1, 4), wkt=wkt, epsg=4326, name="wkt.las")
    crs = pcr.read_point_cloud_info(path).crs                                     # the WKT record wins over the GeoKeys
    assert crs.wkt == wkt and pcr.crs_epsg(crs) == 32633
    path, *_ = make_file(tmp_path, 1, 0, name="nocrs.las")
    assert not pcr.read_point_cloud_info(path).crs.is_valid()
    # LAS 1.4: the 64-bit count with a legacy count of 0
    path, *_ = make_file(tmp_path, 7, 0, version=(1, 4), count64_only=True, name="c64.las")
    assert pcr.read_point_cloud_info(path).num_points == N and pcr.read_point_cloud(path).count() == N
    # magic, not extension
    other = str(tmp_path / "tile.bin")
    shutil.copy(path, other)
    assert pcr.read_point_cloud(other).count() == N
    assert pcr.PointCloudReader.open(other).format() == pcr.PointCloudFormat.LAS


def tampered(tmp_path, src, name, edits=(), truncate=None):
    data = bytearray(open(src, "rb").read())
    for off, fmt, value in edits:
        struct.pack_into(fmt, data, off, value)
    if truncate is not None:
        data = data[:truncate]
    path = str(tmp_path / name)
    open(path, "wb").write(bytes(data))
    return path


def test_errors(tmp_path):
    src, *_ = make_file(tmp_path, 1, 0, epsg=32633)
    size = os.path.getsize(src)
    cases = [
        ("sig.las", [(0, "<4s", b"LASX")], None, "invalid signature"),
        ("hsize.las", [(94, "<H", 65535)], None, "header size"),
        ("doff.las", [(96, "<I", size + 1)], None, "offset to point data"),
        ("trunc.las", [], size - 1, "truncated"),
        ("count.las", [(107, "<I", N + 1)], None, "truncated"),
        ("reclen.las", [(105, "<H", 27)], None, "record length 27"),
        ("fmt11.las", [(104, "<B", 11)], None, "point format 11"),
        ("laz.las", [(104, "<B", 0x81)], None, "not yet implemented"),
        ("laz6.las", [(104, "<B", 0x41)], None, "not yet implemented"),
        ("vlr.las", [(227 + 20, "<H", 60000)], None, "variable length record"),
        ("nvlr.las", [(100, "<I", 2)], None, "variable length record"),
        ("short.las", [], 100, "shorter than a LAS header"),
    ]
    for name, edits, truncate, message in cases:
        bad = tampered(tmp_path, src, name, edits, truncate)
        with pytest.raises(RuntimeError, match=message):
            pcr.read_point_cloud_info(bad)
        with pytest.raises(RuntimeError):
            pcr.read_point_cloud(bad)
        with pytest.raises(RuntimeError, match=message):
            pcr.read_las(bad)
        with pytest.raises(RuntimeError, match=message):
            pcr.PointCloudReader.open(bad)
    with pytest.raises(RuntimeError, match="'colour' is not a channel"):
        pcr.read_las(src, channels=["z", "colour"])
    with pytest.raises(RuntimeError, match="point format 1 has no channel 'red'"):
        pcr.read_las(src, channels=["red"])
    with pytest.raises(RuntimeError, match="point format 1 has no channel 'nir'"):
        pcr.PointCloudReader.open(src, channels=["nir"])
    with pytest.raises(RuntimeError, match="not yet implemented"):
        pcr.read_point_cloud_info(str(tmp_path / "a.laz"))
    with pytest.raises(RuntimeError, match="not yet implemented"):
        pcr.read_las(str(tmp_path / "a.laz"))
    with pytest.raises(RuntimeError, match="failed to open LAS file.*not yet implemented"):
        pcr.read_point_cloud_info(str(tmp_path / "missing.las"))
    with pytest.raises(RuntimeError, match="not yet implemented"):
        pcr.write_point_cloud(str(tmp_path / "w.las"), pcr.read_point_cloud(src), pcr.PointCloudFormat.LAS)


# ---- ExecutionMode.CPU: ingest_file of a .las == ingest of the model cloud ------------------------------------------------------
W, H = 64, 48


def spec(channel, rtype, ts=""):
    r = pcr.ReductionSpec()
    r.value_channel, r.type = channel, rtype
    if ts:
        r.timestamp_channel = ts
    return r


def config(mode, reductions, filter_class=None, origin=0.0):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = mode
    cfg.reductions = reductions
    cfg.las_gps_time_origin = origin
    if filter_class is not None:
        f = pcr.FilterSpec()
        f.add("classification", pcr.CompareOp.Equal, float(filter_class))
        cfg.filter = f
    return cfg


def grid_file(tmp_path, fmt=1, n=5000, name="grid.las", **kw):
    """n points inside the W x H grid (scale 0.001), classification 0..4."""
    rng = np.random.default_rng(77)
    fields = LC.make_fields(fmt, n, rng)
    fields["X"] = rng.integers(1000, (W - 1) * 1000, n).astype(np.int32)
    fields["Y"] = rng.integers(1000, (H - 1) * 1000, n).astype(np.int32)
    fields["Z"] = rng.integers(-5000, 90000, n).astype(np.int32)
    if fmt <= 5:
        fields["b15"] = (np.arange(n) % 5).astype(np.uint8)
    else:
        fields["classification"] = (np.arange(n) % 5).astype(np.uint8)
    fields["gps_time"] = 3.2e8 + rng.uniform(0.0, 5000.0, n)
    rec = LC.pack_records(fmt, fields)
    scale, offset = (0.001, 0.001, 0.001), (0.0, 0.0, 0.0)
    path = str(tmp_path / name)
    LC.write_las(path, fmt, rec, scale, offset, **kw)
    return path, fields, scale, offset


def model_cloud(want, names, lo=0, hi=None):
    hi = len(want["x"]) if hi is None else hi
    c = pcr.PointCloud.create(max(hi - lo, 1))
    c.resize(hi - lo)
    c.set_x_array(want["x"][lo:hi])
    c.set_y_array(want["y"][lo:hi])
    for name in names:
        c.add_channel(name, pcr.DataType.Float32)
        c.set_channel_array_f32(name, want[name][lo:hi])
    return c


def bands(pipe):
    pipe.finalize()
    g = pipe.result()
    return [np.array(g.band_array(b)) for b in range(g.num_bands())]


def assert_same_bands(a, b, what):
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), f"{what}: band {k} differs in {(p.view(np.uint32) != q.view(np.uint32)).sum()} cells"


@pytest.mark.parametrize("case", ["plain", "filter", "most_recent"])
def test_cpu_ingest_file_equals_ingest_of_model(tmp_path, case):
    path, fields, scale, offset = grid_file(tmp_path)
    origin = 3.2e8 if case == "most_recent" else 0.0
    want = LC.expected(1, fields, scale, offset, origin)
    T = pcr.ReductionType
    if case == "most_recent":
        red, names = [spec("z", T.MostRecent, ts="gps_time"), spec("intensity", T.Max)], ["z", "gps_time", "intensity"]
    else:
        red, names = [spec("z", T.Average), spec("z", T.Max), spec("intensity", T.Count)], ["z", "intensity"]
    flt = 2 if case == "filter" else None
    if flt is not None:
        names = names + ["classification"]
    chunk = 1500
    a = pcr.Pipeline.create(config(pcr.ExecutionMode.CPU, red, flt, origin))
    assert a.engine() == "host"
    assert a.ingest_file(path, chunk) == len(want["x"])
    b = pcr.Pipeline.create(config(pcr.ExecutionMode.CPU, red, flt, origin))
    for lo in range(0, len(want["x"]), chunk):                                 # the same chunks: Average sums in the same order
        b.ingest(model_cloud(want, names, lo, min(lo + chunk, len(want["x"]))))
    assert_same_bands(bands(a), bands(b), case)
    c = pcr.Pipeline.create(config(pcr.ExecutionMode.CPU, [spec("red", T.Max)]))
    with pytest.raises(RuntimeError, match="point format 1 has no channel 'red'"):
        c.ingest_file(path, chunk)


# ---- the header parser under AddressSanitizer + UBSan, in a program of its own ---------------------------------------------------
def test_header_parser_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    host = os.path.join(PKG, "host")
    exe = str(tmp_path / "las_header_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(host, "include"), "-I", os.path.join(host, "src"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "las_header_san.cpp"),
                    os.path.join(host, "src", "core.cpp"), "-L", os.path.join(PKG, "lib"), "-lpcr_hip", "-pthread",
                    f"-Wl,-rpath,{os.path.join(PKG, 'lib')}", "-o", exe], check=True)
    seeds = []
    for k, (fmt, kw) in enumerate([(1, dict(epsg=32633)), (7, dict(version=(1, 4), wkt="PROJCS[\"x\"]", epsg=4326)),
                                   (3, dict()), (6, dict(version=(1, 4), count64_only=True))]):
        path, *_ = make_file(tmp_path, fmt, 0, n=50, name=f"seed{k}.las", **kw)
        seeds.append(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe, str(tmp_path)] + seeds, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "header parser survived" in out.stdout
