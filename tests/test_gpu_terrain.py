"""The terrain bands on the MI355X: pcr_hip_terrain through the C-ABI (every product alone and together, both edge modes, rows
on 16 bytes and not, windows of strided planes between sentinels), behind pcr.terrain on Device grids, and the HIP engine's
PipelineConfig.terrain.  Everything BIT FOR BIT against the host loop, which tests/test_terrain.py holds to the NumPy model of
the contract."""
import ctypes as C

import numpy as np
import pytest

import ground_filter_common as G
import overviews_common as M
import pcr
import terrain_common as T
from conftest import load_cabi

pytestmark = pytest.mark.gpu

P = pcr.TerrainProduct
# (rows, cols).  The kernel's tile is 64 columns x 32 rows: the issue's list (one below, on and one above 64 cells both ways)
# plus one below, on and one above 32 rows
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 2), (3, 3), (31, 63), (32, 64), (33, 63), (34, 64), (35, 65), (67, 129), (70, 130), (130, 300)]
SETS = [[p] for p in T.PRODUCTS] + [[P.Hillshade, P.SlopeDegrees, P.Aspect], list(T.PRODUCTS)]
SENTINEL = np.float32(-12345.5)


def device_terrain(a, products, sp=None, cx=1.0, cy=-1.0, offset=0, stride=None):
    """pcr_hip_terrain on `a` as a window at float `offset` of a plane with rows `stride` floats apart; every dst is the same
    window of its own plane of sentinels.  Returns [len(products), h, w]; asserts that nothing was stored outside a window and
    that the source is unchanged."""
    A = load_cabi()
    L = A.lib()
    sp = sp or pcr.TerrainSpec()
    h, w = a.shape
    stride = stride or w
    n = offset + (h - 1) * stride + w + 3
    idx = offset + np.arange(h)[:, None] * stride + np.arange(w)[None, :]
    inside = np.zeros(n, bool)
    inside[idx] = True
    plane = np.full(n, SENTINEL, np.float32)
    plane.view(np.uint32)[idx] = a.view(np.uint32)
    src = A.DeviceBuffer.from_numpy(plane)
    outs = [A.DeviceBuffer.from_numpy(np.full(n, SENTINEL, np.float32)) for _ in products]
    k = len(products)
    ids = (C.c_int * k)(*[int(p) for p in products])
    dsts = (C.c_void_p * k)(*[o.ptr.value + 4 * offset for o in outs])
    strides = (C.c_int64 * k)(*([stride] * k))
    sin_alt, ls, lc = pcr.terrain_light(sp.azimuth, sp.altitude)
    A.check(L.pcr_hip_terrain(C.c_void_p(src.ptr.value + 4 * offset), w, h, stride, k, ids, dsts, strides, cx, cy, sp.z_factor,
                              1 if sp.compute_edges else 0, sin_alt, ls, lc, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = []
    for o in outs:
        flat = o.to_numpy()
        assert (flat[~inside] == SENTINEL).all(), "a store outside dst's window"
        got.append(flat[idx])
    M.bits_equal(src.to_numpy(), plane, "the source is only read")
    return np.stack(got)


def check_device(a, products, what, sp=None, cx=1.0, cy=-1.0, **kw):
    want = T.host(a, products, sp, cx, cy)
    got = device_terrain(a, products, sp, cx, cy, **kw)
    for k, p in enumerate(products):
        T.bits_equal(got[k], want[k], f"{what}: {T.NAMES[int(p)]}")
        assert (got[k].view(np.uint32)[np.isnan(got[k])] == 0x7FC00000).all(), "every NaN is the one NaN"
    return got


@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_product_set_equals_the_host_loop(shape, edges):
    h, w = shape
    a = T.hills(w, h, seed=w * 1000 + h, nan_fraction=0.1)
    for products in SETS:
        check_device(a, products, f"{h}x{w} edges={edges}", T.spec(compute_edges=edges))


@pytest.mark.parametrize("stride_extra", [0, 5])
@pytest.mark.parametrize("offset", [0, 3])                      # rows on 16 bytes (with stride_extra 0 and w % 4 == 0) and not
@pytest.mark.parametrize("shape", [(34, 64), (35, 65), (70, 132)])
def test_windows_of_strided_planes(shape, offset, stride_extra):
    h, w = shape
    a = T.hills(w, h, seed=7 + offset + stride_extra, nan_fraction=0.2)
    for products in SETS[-2:]:
        for edges in (False, True):
            check_device(a, products, f"{h}x{w} offset {offset} stride {w + stride_extra}", T.spec(compute_edges=edges),
                         offset=offset, stride=w + stride_extra)
    # rows on 16 bytes with a stride that is a multiple of 4 beyond the width: the vector variant on a window
    if offset == 0 and stride_extra == 0:
        check_device(a, list(T.PRODUCTS), "stride w + 8", offset=4, stride=(w + 3) // 4 * 4 + 8)


@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("nan_fraction", [0.0, 0.3])
def test_special_values(nan_fraction, edges):
    # +-Inf, FLT_MAX, -0.0, denormals and NaNs of several payloads (a signalling one among them)
    a = M.values(129, 67, seed=21, nan_fraction=nan_fraction)
    check_device(a, list(T.PRODUCTS), f"values nan={nan_fraction}", T.spec(compute_edges=edges))
    check_device(a, list(T.PRODUCTS), "values, other parameters", T.spec(compute_edges=edges, z_factor=-3.5, azimuth=10.0, altitude=80.0),
                 cx=-0.25, cy=4.0)


def test_degenerate_bands():
    for edges in (False, True):
        sp = T.spec(compute_edges=edges)
        got = check_device(np.full((70, 130), np.nan, np.float32), list(T.PRODUCTS), "all NaN", sp)
        assert np.isnan(got).all()
        got = check_device(np.full((70, 130), 3.25, np.float32), list(T.PRODUCTS), "flat", sp)
        inner = got[:, 1:-1, 1:-1]
        flat_hs = np.float32(1.0 + 254.0 * pcr.terrain_light()[0])
        for k, want in enumerate((0.0, 0.0, -1.0, flat_hs, 0.0, 0.0, 0.0)):
            assert (inner[k] == np.float32(want)).all(), T.NAMES[k]
        assert np.isnan(got[:, 0, :]).all() != edges


def test_sqrt_and_division_are_correctly_rounded():
    """The contract takes binary64 sqrt and / on the device for correctly rounded: a band whose s2 covers 2^-40 .. 2^40 densely
    (every power of two in between has cells), through every product that uses either."""
    a = T.ramp(300, 130)
    with np.errstate(all="ignore"):
        pct = T.terrain(a, [P.SlopePercent])[0].astype(np.float64)
    e = np.floor(np.log2((pct[np.isfinite(pct) & (pct > 0)] / 100.0) ** 2)).astype(int)
    assert set(range(-40, 41)) <= set(e.tolist()), "the ramp covers every binade of s2 from 2^-40 to 2^40"
    for z in (1.0, 0.37):
        check_device(a, [P.SlopeDegrees, P.SlopePercent, P.Aspect, P.Hillshade], f"ramp z={z}", T.spec(z_factor=z))
    check_device(np.ascontiguousarray(a.T), [P.SlopeDegrees, P.SlopePercent, P.Aspect, P.Hillshade], "ramp, transposed")


def test_free_function_on_a_device_grid():
    a, b = T.hills(130, 70, 31, 0.05), M.values(130, 70, 32)
    g = T.make_grid([a, b])
    sp = T.spec(z_factor=2.0, compute_edges=True, azimuth=200.0, altitude=60.0)
    for band, order in ((0, list(T.PRODUCTS)), (1, [P.TPI, P.Hillshade])):
        host = pcr.terrain(g, band, order, sp, 2.0, -0.5)
        dev = pcr.terrain(g.to(pcr.MemoryLocation.Device), band, order, sp, 2.0, -0.5)
        assert dev.location() == pcr.MemoryLocation.Device
        names = [dev.band_desc(k).name for k in range(dev.num_bands())]
        assert names == [host.band_desc(k).name for k in range(host.num_bands())] == [T.NAMES[int(p)] for p in order]
        for k, (x, y) in enumerate(zip(T.grid_bands(dev.to_host()), T.grid_bands(host))):
            M.bits_equal(x, y, f"band {band}: {names[k]}")
    with pytest.raises(RuntimeError, match="duplicate product"):
        pcr.terrain(g.to(pcr.MemoryLocation.Device), 0, [P.TRI, P.TRI])


# ---- the HIP engine's PipelineConfig.terrain -----------------------------------------------------------------------------------
WP, HP, NP, RP = 256, 192, 30_000, 3
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU
LOCATIONS = [pcr.MemoryLocation.Host, pcr.MemoryLocation.Device]
NEW = ["dtm_hillshade", "dtm_slope", "mean_aspect", "dtm_roughness", "mean_slope_percent", "hag_tpi", "dtm_hillshade_east"]


def pipeline_cfg(mode, location=pcr.MemoryLocation.Host, terrain=True, W=WP, H=HP, radius=RP):
    """ground + fill_nodata_radius + terrain on `dtm`, on an Average band and on `hag`."""
    cfg = G.pipeline_cfg(W, H, mode, radius=radius)
    r = pcr.ReductionSpec()
    r.value_channel, r.type, r.output_band_name = "value", pcr.ReductionType.Average, "mean"
    cfg.reductions = list(cfg.reductions) + [r]
    cfg.result_location = location
    if terrain:
        cfg.terrain = [T.band_cfg("dtm", P.Hillshade), T.band_cfg("dtm", P.SlopeDegrees), T.band_cfg("mean", P.Aspect),
                       T.band_cfg("dtm", P.Roughness, compute_edges=True), T.band_cfg("mean", P.SlopePercent, z_factor=2.0),
                       T.band_cfg("hag", P.TPI), T.band_cfg("dtm", P.Hillshade, "dtm_hillshade_east", azimuth=90.0, altitude=30.0)]
    return cfg


def create(cfg, engine="hip"):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == engine
    return pipe


def result_bands(pipe):
    res = pipe.result()
    return G.grid_bands(res if res.location() == pcr.MemoryLocation.Host else res.to_host())


def names_of(pipe):
    res = pipe.result()
    return [res.band_desc(b).name for b in range(res.num_bands())]


@pytest.fixture(scope="module")
def pipe_case():
    c1, c2 = G.cloud(WP, HP, NP, seed=81), G.cloud(WP, HP, NP, seed=82)
    host = create(pipeline_cfg(CPU), "host")
    want = []
    for c in (c1, c2):
        host.ingest(c)
        host.finalize()
        want.append(G.grid_bands(host.result()))
    assert names_of(host) == list(G.BANDS) + ["mean", "dtm", "hag"] + NEW
    return c1, c2, want


@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_equals_the_host_engine(pipe_case, location, wait):
    c1, c2, want = pipe_case
    pipe = create(pipeline_cfg(GPU, location))
    A = load_cabi()
    for k, c in enumerate((c1, c2)):                              # finalize() twice with an ingest between
        pipe.ingest(c)
        if wait:
            pipe.finalize()
        else:
            pipe.finalize_async()
            pipe.synchronize()
        assert names_of(pipe) == list(G.BANDS) + ["mean", "dtm", "hag"] + NEW
        got = result_bands(pipe)
        assert len(got) == 13
        # The engines add a cell's points in different orders, so their Average bands agree to rounding only (a handful of
        # points per cell, each addition within 2^-24 relative: 1e-6); Min, Max, Count, the DTM and hag are exact.  So every
        # band that has no Average in its ancestry is the host engine's bit for bit, and every terrain band is the host loop
        # of ITS OWN pipeline's source band bit for bit.
        names = names_of(pipe)
        for b in range(13):
            if "mean" in names[b]:
                continue
            M.bits_equal(got[b], want[k][b], f"finalize {k + 1}, band {b}")
        assert (np.isnan(got[3]) == np.isnan(want[k][3])).all()
        np.testing.assert_allclose(got[3], want[k][3], rtol=1e-6, atol=0.0, equal_nan=True)
        own = T.expect_bands(dict(zip(names[:6], got[:6])), pipeline_cfg(GPU, location))
        for b in range(6, 13):                                    # result_band_device() answers for the new bands
            M.bits_equal(got[b], own[b - 6], f"finalize {k + 1}, band {b} is the host loop of the source as it leaves")
            back = np.empty((HP, WP), np.float32)
            A.check(A.lib().pcr_hip_memcpy_d2h(back.ctypes.data, C.c_void_p(pipe.result_band_device_ptr(b)), back.nbytes, None))
            A.check(A.lib().pcr_hip_stream_synchronize(None))
            M.bits_equal(back, got[b], f"finalize {k + 1}, result_band_device {b}")
        assert pipe.result_band_device_ptr(13) == 0
    assert np.isnan(got[6]).any() and not np.isnan(got[6]).all()


@pytest.mark.parametrize("location", LOCATIONS)
def test_an_empty_list_changes_nothing(pipe_case, location):
    c1 = pipe_case[0]
    bands = []
    for cfg in (pipeline_cfg(GPU, location, terrain=False), pipeline_cfg(GPU, location, terrain=False)):
        if bands:
            cfg.terrain = []
        pipe = create(cfg)
        pipe.ingest(c1)
        pipe.finalize()
        bands.append((names_of(pipe), result_bands(pipe)))
    assert bands[0][0] == bands[1][0] == list(G.BANDS) + ["mean", "dtm", "hag"]
    with_terrain = create(pipeline_cfg(GPU, location))
    with_terrain.ingest(c1)
    with_terrain.finalize()
    other = result_bands(with_terrain)
    for b in range(6):
        M.bits_equal(bands[0][1][b], bands[1][1][b], f"band {b}")
        M.bits_equal(bands[0][1][b], other[b], f"band {b} is the band of the pipeline with terrain bands")


@pytest.mark.parametrize("location", LOCATIONS)
def test_without_a_ground_plan_the_first_terrain_band_is_not_filled(location):
    """fill_nodata_radius > 0 and no ground plan: the band behind the outputs is then the first terrain band, not the DTM, and
    leaves as the kernel stored it (the table of leaving bands once took it for the DTM and filled it: seed 0 of the
    operation-sequence fuzz).  Sparse points, so that no-data cells lie within the radius of valid ones; 72 x 40 is more than
    one terrain tile each way."""
    W, H = 72, 40
    cfg = G.pipeline_cfg(W, H, GPU, ground=False, radius=2)
    cfg.result_location = location
    cfg.terrain = [T.band_cfg(G.BANDS[2], P.TRI, compute_edges=True), T.band_cfg(G.BANDS[1], P.SlopeDegrees, compute_edges=True),
                   T.band_cfg(G.BANDS[2], P.Roughness)]
    pipe = create(cfg)
    pipe.ingest(G.cloud(W, H, 700, seed=84))
    pipe.finalize()
    names, got = names_of(pipe), result_bands(pipe)
    assert names == list(G.BANDS) + [f"{G.BANDS[2]}_tri", f"{G.BANDS[1]}_slope", f"{G.BANDS[2]}_roughness"]
    want = T.expect_bands(dict(zip(names[:3], got[:3])), cfg)
    for b in range(3, 6):
        M.bits_equal(got[b], want[b - 3], f"band {b} ({names[b]}) is the host loop of the source as it leaves")
    # with compute_edges a cell is no data exactly where its source is: the Count band is not filled, so neither is its TRI
    count_nan = np.isnan(got[2])
    assert np.array_equal(np.isnan(got[3]), count_nan) and count_nan[:, :int(W * 0.9)].sum() > 200
    assert np.isnan(got[0]).sum() < count_nan.sum()              # (the fill did run on the Min band)


@pytest.mark.parametrize("location", LOCATIONS)
def test_geotiff_and_overview_levels_hold_the_new_bands(tmp_path, location):
    Wc, Hc = 520, 512                                              # write_cog's rule gives a level only from 512 cells a side
    pts = G.cloud(Wc, Hc, 200_000, seed=83)
    cfg = pipeline_cfg(GPU, location, W=Wc, H=Hc, radius=2)
    cfg.output_path, cfg.write_cog = str(tmp_path / "t.tif"), True
    pipe = create(cfg)
    pipe.ingest(pts)
    pipe.finalize()
    got = result_bands(pipe)
    assert pcr.read_geotiff_overviews(cfg.output_path) == [(260, 256)]
    assert pcr.read_geotiff_band_names(cfg.output_path) == names_of(pipe)
    levels = T.grid_bands(pcr.build_overviews(T.make_grid(got), 1)[0])
    sources = dict(zip(names_of(pipe)[:6], got[:6]))
    want_new = T.expect_bands(sources, cfg)
    for b in range(13):
        if b >= 6:
            T.bits_equal(got[b], want_new[b - 6], f"band {b}")
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), got[b], f"file band {b}")
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), levels[b], f"file band {b} level 1")
        M.bits_equal(levels[b], M.down(got[b]), f"level 1 of band {b}")
