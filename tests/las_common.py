"""What the LAS tests share: a LAS writer and the expected cloud, both from the ASPRS LAS 1.4 (R15) layout restated in NumPy
structured dtypes -- no code in common with the C++ header parser or the record decoder.

    fields  = make_fields(fmt, n, rng)           raw record fields (X, Y, Z, the packed bytes, ...), edge values included
    records = pack_records(fmt, fields, extra)   structured array, itemsize = the format's minimum + extra
    write_las(path, fmt, records, scale, offset, version=(1, 2) | (1, 4), wkt=..., epsg=...)
    expected(fmt, fields, scale, offset, origin) name -> array: x, y Float64, every channel of the format Float32
"""
import struct

import numpy as np

CHANNELS = ("z", "intensity", "return_number", "number_of_returns", "classification", "withheld", "overlap",
            "scan_angle", "user_data", "point_source_id", "gps_time", "red", "green", "blue", "nir")
MIN_LENGTH = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}
HAS_GPS = {1, 3, 4, 5, 6, 7, 8, 9, 10}
HAS_RGB = {2, 3, 5, 7, 8, 10}
HAS_NIR = {8, 10}
HAS_WAVE = {4, 5, 9, 10}
_WAVE = [("wave_index", "u1"), ("wave_offset", "<u8"), ("wave_size", "<u4"), ("wave_location", "<f4"),
         ("wave_xt", "<f4"), ("wave_yt", "<f4"), ("wave_zt", "<f4")]


def channels_of(fmt):
    names = list(CHANNELS[:10])
    if fmt in HAS_GPS:
        names.append("gps_time")
    if fmt in HAS_RGB:
        names += ["red", "green", "blue"]
    if fmt in HAS_NIR:
        names.append("nir")
    return names


def point_dtype(fmt, extra=0):
    f = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2"), ("b14", "u1"), ("b15", "u1")]
    if fmt <= 5:
        f += [("scan_angle", "i1"), ("user_data", "u1"), ("point_source_id", "<u2")]
    else:
        f += [("classification", "u1"), ("user_data", "u1"), ("scan_angle", "<i2"), ("point_source_id", "<u2")]
    if fmt in HAS_GPS:
        f.append(("gps_time", "<f8"))
    if fmt in HAS_RGB:
        f += [("red", "<u2"), ("green", "<u2"), ("blue", "<u2")]
    if fmt in HAS_NIR:
        f.append(("nir", "<u2"))
    if fmt in HAS_WAVE:
        f += _WAVE
    if extra:
        f.append(("extra", "u1", (extra,)))
    dt = np.dtype(f)                      # packed: no alignment padding
    assert dt.itemsize == MIN_LENGTH[fmt] + extra
    return dt


def make_fields(fmt, n, rng, gps_base=3.2e8):
    """Random raw fields with the edge values up front: X of INT32_MIN / INT32_MAX, intensity 0 / 65535, every value of the
    two packed bytes (n >= 256), classification 31 / 255, negative scan angles, GPS times near gps_base."""
    i32 = np.iinfo(np.int32)
    f = {
        "X": rng.integers(-2_000_000, 2_000_000, n).astype(np.int32),
        "Y": rng.integers(-2_000_000, 2_000_000, n).astype(np.int32),
        "Z": rng.integers(-50_000, 900_000, n).astype(np.int32),
        "intensity": rng.integers(0, 65536, n).astype(np.uint16),
        "b14": (np.arange(n) % 256).astype(np.uint8),
        "b15": ((np.arange(n) * 7 + 3) % 256).astype(np.uint8),
        "user_data": rng.integers(0, 256, n).astype(np.uint8),
        "point_source_id": rng.integers(0, 65536, n).astype(np.uint16),
        "gps_time": gps_base + rng.uniform(0.0, 1.0e4, n),
        "red": rng.integers(0, 65536, n).astype(np.uint16),
        "green": rng.integers(0, 65536, n).astype(np.uint16),
        "blue": rng.integers(0, 65536, n).astype(np.uint16),
        "nir": rng.integers(0, 65536, n).astype(np.uint16),
        "classification": rng.integers(0, 256, n).astype(np.uint8),         # formats 6-10 (0-5: the low bits of b15)
    }
    f["scan_angle"] = (rng.integers(-128, 128, n).astype(np.int8) if fmt <= 5
                       else rng.integers(-30_000, 30_001, n).astype(np.int16))
    edge = [("X", [i32.min, i32.max, 0, -1]), ("Y", [i32.max, i32.min, 1, 0]), ("Z", [i32.min, i32.max, 0, -1]),
            ("intensity", [0, 65535]), ("classification", [255, 12, 0]), ("user_data", [0, 255]),
            ("point_source_id", [0, 65535]), ("red", [0, 65535]), ("nir", [65535, 0]),
            ("scan_angle", [-128, 127, -1] if fmt <= 5 else [-30000, 30000, -1, -32768, 32767]),
            ("gps_time", [gps_base, gps_base + 0.001, gps_base - 17.25, 0.0])]
    for name, vals in edge:
        k = min(len(vals), n)
        f[name][:k] = np.asarray(vals[:k]).astype(f[name].dtype)
    if fmt <= 5 and n > 40:
        f["b15"][33:36] = [31, 12, 12 | 0x80]          # classification 31; 12 = overlap, with and without the withheld bit
    return f


def pack_records(fmt, fields, extra=0, rng=None):
    dt = point_dtype(fmt, extra)
    n = len(fields["X"])
    rec = np.zeros(n, dtype=dt)
    rng = rng or np.random.default_rng(5)
    for name in dt.names:
        if name in fields:
            rec[name] = fields[name]
        elif name.startswith("wave_") or name == "extra":                   # bytes a reader must skip: noise
            raw = rng.integers(0, 256, (n, dt[name].itemsize), dtype=np.uint8)
            rec[name] = raw.view(dt[name].base).reshape(rec[name].shape) if name != "extra" else raw
    return rec


def expected(fmt, fields, scale, offset, origin=0.0):
    f = fields
    f64 = np.float64
    out = {"x": f["X"].astype(f64) * f64(scale[0]) + f64(offset[0]),
           "y": f["Y"].astype(f64) * f64(scale[1]) + f64(offset[1]),
           "z": (f["Z"].astype(f64) * f64(scale[2]) + f64(offset[2])).astype(np.float32),
           "intensity": f["intensity"].astype(np.float32),
           "user_data": f["user_data"].astype(np.float32),
           "point_source_id": f["point_source_id"].astype(np.float32)}
    b14, b15 = f["b14"].astype(np.uint32), f["b15"].astype(np.uint32)
    if fmt <= 5:
        cls = b15 & 31
        out["return_number"] = (b14 & 7).astype(np.float32)
        out["number_of_returns"] = ((b14 >> 3) & 7).astype(np.float32)
        out["classification"] = cls.astype(np.float32)
        out["withheld"] = ((b15 >> 7) & 1).astype(np.float32)
        out["overlap"] = (cls == 12).astype(np.float32)
        out["scan_angle"] = f["scan_angle"].astype(np.float32)
    else:
        out["return_number"] = (b14 & 15).astype(np.float32)
        out["number_of_returns"] = ((b14 >> 4) & 15).astype(np.float32)
        out["classification"] = f["classification"].astype(np.float32)
        out["withheld"] = ((b15 >> 2) & 1).astype(np.float32)
        out["overlap"] = ((b15 >> 3) & 1).astype(np.float32)
        out["scan_angle"] = (f["scan_angle"].astype(f64) * f64(0.006)).astype(np.float32)
    if fmt in HAS_GPS:
        out["gps_time"] = (f["gps_time"].astype(f64) - f64(origin)).astype(np.float32)
    if fmt in HAS_RGB:
        for c in ("red", "green", "blue"):
            out[c] = f[c].astype(np.float32)
    if fmt in HAS_NIR:
        out["nir"] = f["nir"].astype(np.float32)
    return out


def geokey_vlr(epsg, geographic=False):
    """GeoKeyDirectory (record 34735): GTModelType + the ProjectedCSType (3072) or GeographicType (2048) key."""
    keys = [(1024, 0, 1, 2 if geographic else 1), (2048 if geographic else 3072, 0, 1, epsg)]
    body = struct.pack("<4H", 1, 1, 0, len(keys)) + b"".join(struct.pack("<4H", *k) for k in keys)
    return vlr("LASF_Projection", 34735, body)


def wkt_vlr(wkt):
    return vlr("LASF_Projection", 2112, wkt.encode() + b"\0")


def vlr(user_id, record_id, body, description=""):
    return (struct.pack("<H16sHH32s", 0, user_id.encode(), record_id, len(body), description.encode()) + body)


def header_bytes(fmt, record_length, n, scale, offset, bounds, version=(1, 2), vlr_bytes=b"", n_vlrs=0, count64_only=False):
    size = {0: 227, 1: 227, 2: 227, 3: 235, 4: 375}[version[1]]
    h = bytearray(size)
    h[0:4] = b"LASF"
    h[24], h[25] = version
    h[26:26 + 13] = b"pcr test file"
    struct.pack_into("<HH", h, 90, 100, 2024)
    struct.pack_into("<HII", h, 94, size, size + len(vlr_bytes), n_vlrs)
    h[104] = fmt
    struct.pack_into("<H", h, 105, record_length)
    legacy = 0 if (count64_only or n >= 2 ** 32) else n
    struct.pack_into("<I", h, 107, legacy)
    struct.pack_into("<3d", h, 131, *scale)
    struct.pack_into("<3d", h, 155, *offset)
    min_x, min_y, max_x, max_y = bounds
    struct.pack_into("<4d", h, 179, max_x, min_x, max_y, min_y)
    if size >= 375:
        struct.pack_into("<Q", h, 247, n)
    return bytes(h)


def write_las(path, fmt, records, scale, offset, version=(1, 2), wkt=None, epsg=None, geographic=False, count64_only=False,
              trailing=b""):
    """Writes the file and returns (header_size, data_offset).  bounds in the header: min / max of the scaled x, y."""
    vl = []
    if wkt is not None:
        vl.append(wkt_vlr(wkt))
    if epsg is not None:
        vl.append(geokey_vlr(epsg, geographic))
    vb = b"".join(vl)
    x = records["X"].astype(np.float64) * scale[0] + offset[0]
    y = records["Y"].astype(np.float64) * scale[1] + offset[1]
    bounds = (x.min(), y.min(), x.max(), y.max()) if len(records) else (0.0, 0.0, 0.0, 0.0)
    hb = header_bytes(fmt, records.dtype.itemsize, len(records), scale, offset, bounds, version, vb, len(vl), count64_only)
    with open(path, "wb") as f:
        f.write(hb + vb + records.tobytes() + trailing)
    return len(hb), len(hb) + len(vb)


def cloud_arrays(cloud, names):
    """x, y and the named channels of a host-resident pcr.PointCloud as a dict of numpy arrays."""
    out = {"x": np.array(cloud.x_array()), "y": np.array(cloud.y_array())}
    for name in names:
        out[name] = np.array(cloud.channel_array_f32(name))
    return out


def assert_bits_equal(got, want, what=""):
    assert sorted(got) == sorted(want), f"{what}: arrays {sorted(got)} != {sorted(want)}"
    for name in want:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype}{g.shape} != {w.dtype}{w.shape}"
        same = g.view(np.uint8).reshape(len(g), -1) == w.view(np.uint8).reshape(len(w), -1) if len(g) else np.ones((0, 1), bool)
        bad = np.flatnonzero(~same.all(axis=1))
        assert bad.size == 0, f"{what} {name}: {bad.size} differ, first at {bad[0]}: {g[bad[0]]!r} != {w[bad[0]]!r}"
