"""Sampling a band at the points of a cloud on the MI355X: pcr_hip_sample_grid against its host twin (which
tests/test_sample_grid.py holds to the NumPy model), pcr.sample_grid on Device clouds, the HIP engine's surface channels --
"derived at ingest == precomputed channel" -- and the two-pass canopy workflow end to end.  Every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import pcr
import reduction_filters_common as RF
import sample_grid_common as SG
import test_sample_grid as CPU
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NEAREST, BILINEAR = SG.NEAREST, SG.BILINEAR
S = RF.S
DEVICE, PINNED = pcr.MemoryLocation.Device, pcr.MemoryLocation.HostPinned
PER_WG = 256 * 4                                                 # points per workgroup: 256 * PCR_HIP_SAMPLE_POINTS_PER_LANE
COUNTS = [1, 63, 64, 65, 255, 256, 257, PER_WG - 1, PER_WG, PER_WG + 1, 2 * PER_WG + 37]
SENTINEL = F32(-777.25)
NORTH = [(n, s) for n, s in SG.surfaces() if n.endswith("north")]


def gpu_config(specs, cfg_filt=(), **kw):
    return RF.make_config("gpu", specs, cfg_filt, SG.PGRID, **kw)


class Arrays:
    """x, y, value in device buffers, each twice: starting on 16 bytes (element 4 of the allocation) and one element off it."""

    def __init__(self, A, x, y, z):
        self.A, self.n = A, x.size
        self.host = dict(x=np.ascontiguousarray(x, F64), y=np.ascontiguousarray(y, F64), z=np.ascontiguousarray(z, F32))
        self.images, self.dev = {}, {}
        for name, a in self.host.items():
            for off in (4, 5):
                img = np.full(self.n + 12, 4321.0, a.dtype)
                img[off:off + self.n] = a
                self.images[name, off] = img
                self.dev[name, off] = A.DeviceBuffer.from_numpy(img)

    def ptr(self, name, off):
        return C.c_void_p(self.dev[name, off].ptr.value + off * self.host[name].itemsize)

    def assert_only_read(self):
        for key, buf in self.dev.items():
            assert np.array_equal(buf.to_numpy().view(np.uint8), self.images[key].view(np.uint8)), f"{key} changed"


def run_kernel(A, g, d_band, stride, arrays, offs, mode, with_value, in_place=False):
    """offs: element offsets (4 or 5) of x, y, value, out.  -> the n outputs; the sentinels around them are checked."""
    L = A.lib()
    n = arrays.n
    ox, oy, oz, oo = offs
    if in_place:
        img = arrays.images["z", oz].copy()
        d_out = A.DeviceBuffer.from_numpy(img)
        out_ptr = z_ptr = C.c_void_p(d_out.ptr.value + oz * 4)
        oo = oz
    else:
        img = np.full(n + 12, SENTINEL, F32)
        d_out = A.DeviceBuffer.from_numpy(img)
        out_ptr = C.c_void_p(d_out.ptr.value + oo * 4)
        z_ptr = arrays.ptr("z", oz) if with_value else None
    A.check(L.pcr_hip_sample_grid(C.byref(g), d_band, stride, arrays.ptr("x", ox), arrays.ptr("y", oy), z_ptr, n, mode, out_ptr, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = d_out.to_numpy()
    assert np.array_equal(got[:oo].view(np.uint32), img[:oo].view(np.uint32)), "a store in front of the outputs"
    assert np.array_equal(got[oo + n:].view(np.uint32), img[oo + n:].view(np.uint32)), "a store behind the outputs"
    return got[oo:oo + n]


@pytest.mark.parametrize("name,s", NORTH, ids=[n for n, _ in NORTH])
def test_kernel_equals_the_host_loop(name, s):
    """Every point count around the kernel's strides, both modes, with and without a value channel, x / y / value / out on 16
    bytes and one element off it, the band a window of a plane of sentinels, the output inside a buffer of sentinels."""
    A = load_cabi()
    g = SG.cabi_grid(A, s)
    stride, off = s.w + 3, 2 * (s.w + 3) + 1                      # the band: rows stride apart, starting inside the plane
    plane = np.full((s.h + 4) * stride, SENTINEL, F32)
    window = plane[off:]
    for r in range(s.h):
        window[r * stride:r * stride + s.w] = s.band[r]
    d_plane = A.DeviceBuffer.from_numpy(plane)
    d_band = C.c_void_p(d_plane.ptr.value + off * 4)
    rng = np.random.default_rng(len(name))
    lx, ly = SG.lattice(s, rng, 0)
    combos = [(4, 4, 4, 4), (5, 4, 4, 4), (4, 5, 4, 4), (4, 4, 5, 4), (4, 4, 4, 5), (5, 5, 5, 5)]
    for n in COUNTS:
        pick = rng.integers(0, lx.size, n)
        jitter = rng.random(n) < 0.5                               # half lattice points, half random ones
        x = np.where(jitter, rng.uniform(s.min_x - 1.0, s.max_x + 1.0, n), lx[pick])
        y = np.where(jitter, rng.uniform(s.min_y - 1.0, s.max_y + 1.0, n), ly[pick])
        z = SG.values_for(n, rng)
        arrays = Arrays(A, x, y, z)
        for mode in (NEAREST, BILINEAR):
            want = {v: SG.host_loop(A, s, x, y, z if v else None, mode, band=window, stride=stride) for v in (False, True)}
            for with_value in (False, True):
                for offs in combos:
                    got = run_kernel(A, g, d_band, stride, arrays, offs, mode, with_value)
                    SG.bits_equal(got, want[with_value], f"{name} n {n} mode {mode} value {with_value} offsets {offs}")
            for oz in (4, 5):                                      # in place: out == value
                got = run_kernel(A, g, d_band, stride, arrays, (4, 4, oz, oz), mode, True, in_place=True)
                SG.bits_equal(got, want[True], f"{name} n {n} mode {mode} in place at offset {oz}")
        arrays.assert_only_read()
    assert np.array_equal(d_plane.to_numpy().view(np.uint32), plane.view(np.uint32)), "the band's plane changed"


@pytest.mark.parametrize("name,s", SG.surfaces(), ids=[n for n, _ in SG.surfaces()])
def test_kernel_on_the_lattice(name, s):
    A = load_cabi()
    g = SG.cabi_grid(A, s)
    rng = np.random.default_rng(sum(map(ord, name)))
    x, y = SG.lattice(s, rng)
    z = SG.values_for(x.size, rng)
    arrays = Arrays(A, x, y, z)
    d_band = A.DeviceBuffer.from_numpy(s.band)
    for mode in (NEAREST, BILINEAR):
        for with_value in (False, True):
            got = run_kernel(A, g, d_band.ptr, s.w, arrays, (4, 4, 4, 4), mode, with_value)
            SG.bits_equal(got, SG.host_loop(A, s, x, y, z if with_value else None, mode), f"{name} mode {mode} value {with_value}")
            SG.bits_equal(got, SG.model(s, x, y, z if with_value else None, mode), f"{name} mode {mode} value {with_value}: the model")


# ---- pcr.sample_grid where the cloud lives -------------------------------------------------------------------------------------
def test_sample_grid_on_device_clouds():
    name, s = SG.surfaces()[8]
    rng = np.random.default_rng(77)
    x, y = SG.lattice(s, rng, 3000)
    z = SG.values_for(x.size, rng)
    host = SG.make_cloud(pcr, x, y, {"z": z})
    pcr.sample_grid(host, SG.pcr_grid(pcr, s), 0, "hag", "z")
    want = np.array(host.channel_array_f32("hag"))
    SG.bits_equal(want, SG.model(s, x, y, z, BILINEAR), "host cloud")
    for grid_loc in (DEVICE, None):                              # a Device grid; a Host grid, whose band is copied across first
        cloud = SG.make_cloud(pcr, x, y, {"z": z}, DEVICE)
        pcr.sample_grid(cloud, SG.pcr_grid(pcr, s, grid_loc, extra_bands=1), 1, "hag", "z")
        back = cloud.to_host()
        SG.bits_equal(back.channel_array_f32("hag"), want, f"Device cloud, grid on {grid_loc}")
        SG.bits_equal(back.channel_array_f32("z"), z, "the value channel is only read")
        pcr.sample_grid(cloud, SG.pcr_grid(pcr, s, grid_loc), 0, "z", "z", pcr.SampleMode.Nearest)      # in place
        SG.bits_equal(cloud.to_host().channel_array_f32("z"), SG.model(s, x, y, z, NEAREST), "in place on the device")
    host2 = SG.make_cloud(pcr, x, y, {"z": z})                   # a Host cloud with a Device grid
    pcr.sample_grid(host2, SG.pcr_grid(pcr, s, DEVICE), 0, "hag", "z")
    SG.bits_equal(host2.channel_array_f32("hag"), want, "Host cloud, Device grid")


# ---- the HIP engine's surface channels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("where", ["host", "pinned", "device"])
def test_hip_pipeline_point_reductions_and_filters(path, where):
    loc = {"host": None, "pinned": PINNED, "device": DEVICE}[where]
    c = SG.dyadic_points(20000, 141)
    got = SG.check_pair(pcr, gpu_config, CPU.POINT_SPECS, CPU.HAG, [(c, CPU.surfs(1))], location=loc, scatter_path=path,
                        what=f"point reductions, path {path}, {where} cloud")
    assert not np.array_equal(np.isnan(got[8]), np.isnan(got[11]))
    if path == 2 and where == "device":                          # ... and the host engine gives the same bands
        want = SG.check_pair(pcr, CPU.cpu_config, CPU.POINT_SPECS, CPU.HAG, [(c, CPU.surfs(1))], what="host engine")
        for b, (u, w) in enumerate(zip(got, want)):
            SG.bits_equal(u, w, f"HIP engine against host engine, band {b}")


def test_hip_pipeline_cfg_filter_two_ingests_and_async():
    c1, c2 = SG.dyadic_points(5000, 142), SG.dyadic_points(3000, 143)
    SG.check_pair(pcr, gpu_config, CPU.POINT_SPECS[:5] + CPU.POINT_SPECS[7:9], CPU.HAG,
                  [(c1, CPU.surfs(2)), (c2, CPU.surfs(5, coarse=True))], cfg_filt=[("hag", "LessEqual", 20.0), ("cls", "NotEqual", 5.0)],
                  location=DEVICE, what="cfg.filter on hag, a new surface between two ingests")
    SG.check_pair(pcr, gpu_config, CPU.POINT_SPECS, CPU.HAG, [(c1, CPU.surfs(2)), (c2, CPU.surfs(2))], location=DEVICE,
                  ingest="ingest_async", what="ingest_async of Device clouds")
    SG.check_pair(pcr, gpu_config, CPU.POINT_SPECS, CPU.HAG, [(c1, CPU.surfs(2))], location=PINNED, ingest="ingest_async",
                  what="ingest_async of a pinned cloud")


def test_hip_pipeline_line_and_gaussian_glyphs():
    c = SG.dyadic_points(3000, 144)
    c["z"] = np.abs(c["z"])
    specs = [S("Sum", ch="hag", glyph=RF.LINE), S("Count", ch="hag", glyph=RF.LINE), S("Count", ch="z", filt=[("hag", "Greater", 2.0)], glyph=RF.LINE)]
    SG.check_pair(pcr, gpu_config, specs, CPU.HAG, [(c, CPU.surfs(3))], location=DEVICE, what="Line groups")        # weights 1: exact sums
    # Gaussian footprints that never overlap (one point every 8 cells, 3 cells of reach): a cell has one contribution, so the
    # bands do not depend on the order the atomics land in
    gx, gy = np.meshgrid(np.arange(4.25, 40.0, 8.0), np.arange(4.5, 24.0, 8.0))
    sparse = dict(x=gx.ravel(), y=gy.ravel(), z=np.linspace(3.0, 40.0, gx.size).astype(F32))
    gauss = dict(kind="gauss", sigma=1.0, maxr=3.0)
    for path in (1, 2):
        SG.check_pair(pcr, gpu_config, [S("Average", ch="hag", glyph=gauss), S("Sum", ch="hag", glyph=gauss)], CPU.HAG[:1],
                      [(sparse, {"hag": SG.dyadic_surface(4)})], location=DEVICE, scatter_path=path, what=f"Gaussian glyph, path {path}")


def test_hip_pipeline_chunked_files(tmp_path):
    CPU.check_las_names_only_hag("gpu", tmp_path, gpu_config)    # LAS: raw records cross PCIe, z is decoded in HBM, hag gathered there
    c = SG.dyadic_points(5000, 145)
    path = str(tmp_path / "cloud.pcrp")
    pcr.write_point_cloud(path, SG.dict_cloud(pcr, c))
    chans, s = CPU.HAG, CPU.surfs(6)
    p = pcr.Pipeline.create(gpu_config(CPU.POINT_SPECS, surface_channels=SG.channel_configs(pcr, chans)))
    SG.set_surfaces(pcr, p, s, DEVICE)                           # (the surfaces given as Device grids)
    assert p.ingest_file(path, 1024) == 5000                     # five chunks, the last one ragged
    p.finalize()
    q = pcr.Pipeline.create(gpu_config(CPU.POINT_SPECS))
    q.ingest(SG.dict_cloud(pcr, SG.with_model_channels(c, chans, s)))
    q.finalize()
    SG.assert_same_pipelines(p, q, "chunked PCRP ingest_file", collections=False)


def test_hip_pipeline_reprojected_cloud():
    CPU.check_reprojected("gpu", DEVICE)
    CPU.check_reprojected("gpu")


def test_channel_bits_equal_the_host_engines():
    """One point per cell: a Min band IS the channel.  Any coordinates, any heights, Bilinear and Nearest."""
    c = SG.one_point_per_cell(146)
    rng = np.random.default_rng(1)
    band = (rng.standard_normal((41, 67)) * 25.0 + 30.0).astype(F32)
    band[rng.random(band.shape) < 0.15] = np.nan
    s = SG.Surface(band, 1.3, 22.9, 0.55, -0.53)
    chans = [("hag", "z", BILINEAR), ("gnd", "", NEAREST)]
    specs = [S("Min", ch="hag"), S("Min", ch="gnd")]
    bands = {}
    for mode, config, loc in (("gpu", gpu_config, DEVICE), ("cpu", CPU.cpu_config, None)):
        p = pcr.Pipeline.create(config(specs, surface_channels=SG.channel_configs(pcr, chans)))
        SG.set_surfaces(pcr, p, {"hag": s, "gnd": s})
        p.ingest(SG.dict_cloud(pcr, c, loc))
        p.finalize()
        assert p.engine() == ("hip" if mode == "gpu" else "host")
        bands[mode] = SG.grid_bands(p)
    want = SG.with_model_channels(c, chans, {"hag": s, "gnd": s})
    for b, name in enumerate(("hag", "gnd")):
        SG.bits_equal(bands["gpu"][b], bands["cpu"][b], f"{name}: HIP engine against host engine")
        SG.bits_equal(bands["gpu"][b].ravel(), want[name], f"{name}: HIP engine against the model")
    assert np.isnan(want["hag"]).any() and np.isfinite(want["hag"]).sum() > 500


def test_refusals_on_the_hip_engine():
    CPU.check_refusals("gpu", gpu_config)


# ---- two passes, end to end ------------------------------------------------------------------------------------------------------
def scene(seed=5):
    """64 x 64 cells of 1 m: a tilted plane of ground returns (class 2), a box building (class 6, 9 m above the plane) and a few
    trees (class 5, first returns up to 14 m up, ground returns under them)."""
    rng = np.random.default_rng(seed)
    n = 30000
    x, y = rng.uniform(0.0, 64.0, n), rng.uniform(0.0, 64.0, n)
    ground = 20.0 + 0.05 * x + 0.03 * y
    z = ground + rng.normal(0.0, 0.02, n)
    cls, ret = np.full(n, 2.0, F32), np.full(n, 1.0, F32)
    box = (x > 20) & (x < 32) & (y > 36) & (y < 46)
    z[box], cls[box] = ground[box] + 9.0, 6.0
    for tx, ty, r, top in ((10.0, 12.0, 4.0, 14.0), (45.0, 20.0, 5.0, 11.0), (50.0, 50.0, 3.5, 8.0), (14.0, 52.0, 3.0, 6.0)):
        d = np.hypot(x - tx, y - ty)
        crown = (d < r) & (rng.random(n) < 0.7)
        z[crown] = ground[crown] + top * (1.0 - (d[crown] / r) ** 2) + 1.0
        cls[crown] = 5.0
        under = (d < r) & ~crown
        ret[under] = 2.0
    return dict(x=x, y=y, z=z.astype(F32), cls=cls, ret=ret)


def test_two_passes_end_to_end():
    g = dict(min_x=0.0, min_y=0.0, max_x=64.0, max_y=64.0, cs=1.0, W=64, H=64, tw=64, th=64)
    c = scene()
    # pass 1: Min of class-2 z -> ground filter -> fill -> dtm, left in HBM
    ground = pcr.GroundFilterConfig()
    ground.source_band = "zmin"
    spec = RF.to_spec(S("Min", ch="z", filt=[("cls", "Equal", 2.0)]))
    spec.output_band_name = "zmin"
    cfg1 = RF.make_config("gpu", [], (), g, ground=ground, fill_nodata_radius=16, result_location=DEVICE)
    cfg1.reductions = [spec]
    p1 = pcr.Pipeline.create(cfg1)
    assert p1 is not None, pcr.pipeline_create_error()
    cloud = SG.dict_cloud(pcr, c, DEVICE)
    p1.ingest(cloud)
    p1.finalize()
    res = p1.result()
    assert res.location() == DEVICE and res.geometry() is not None
    dtm_band = res.band_index("dtm")
    dtm = np.array(res.to_host().band_array(dtm_band))
    assert not np.isnan(dtm).any(), "the filled DTM covers the building and the crowns"
    truth = 20.0 + 0.05 * (np.arange(64) + 0.5)[None, :] + 0.03 * (64.0 - (np.arange(64) + 0.5))[:, None]
    assert np.abs(dtm - truth).max() < 0.6, "... with the plane"
    # pass 2: hag from the DTM straight out of result(); the CHM, the returns above 2 m, all returns
    specs = [S("Max", ch="hag", filt=[("ret", "Equal", 1.0)]), S("Count", ch="z", filt=[("hag", "Greater", 2.0)]), S("Count", ch="z")]
    chans = [("hag", "z", BILINEAR)]
    p2 = pcr.Pipeline.create(RF.make_config("gpu", specs, (), g, surface_channels=SG.channel_configs(pcr, chans)))
    assert p2 is not None, pcr.pipeline_create_error()
    p2.set_surface("hag", res, dtm_band)
    p2.ingest(cloud)
    p2.finalize()
    got = SG.grid_bands(p2)
    # the model: the contract's channel from the DTM's bits, folded per cell with NumPy
    hag = SG.model(SG.Surface(dtm, 0.0, 64.0, 1.0, -1.0), c["x"], c["y"], c["z"], BILINEAR)
    cell = RF.cells_of(g, c["x"], c["y"])
    assert (cell >= 0).all() and not np.isnan(hag).any()
    chm = np.full(64 * 64, -np.inf, F32)
    first = c["ret"] == 1.0
    np.maximum.at(chm, cell[first], hag[first])
    chm[np.isinf(chm)] = np.nan
    above = np.bincount(cell[hag > 2.0], minlength=64 * 64).astype(F32)
    every = np.bincount(cell, minlength=64 * 64).astype(F32)
    SG.bits_equal(got[0].ravel(), SG.canonical(chm), "CHM")
    SG.bits_equal(got[1].ravel(), SG.canonical(np.where(above > 0, above, np.nan)), "Count of returns above 2 m")
    SG.bits_equal(got[2].ravel(), SG.canonical(np.where(every > 0, every, np.nan)), "Count of all returns")
    assert 8.0 < np.nanmax(got[0][20:26, 22:30]) < 10.0, "the building stands 9 m above the DTM"
    assert np.nanmax(got[0]) > 12.0, "the tallest tree"
    cover = np.nan_to_num(got[1]) / got[2]
    assert cover[20:26, 22:30].min() == 1.0 and np.nanmin(cover) == 0.0
