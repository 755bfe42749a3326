"""The terrain bands without a GPU: the host loop against the NumPy model of the contract (tests/terrain_common.py) bit for
bit, known answers on planes, the accuracy of atan_deg against binary64, the strict-mode masks, pcr.terrain on Host grids, the
host-engine pipeline's PipelineConfig.terrain (order of the steps, GeoTIFF, overview level, second finalize), the create
errors, the argument errors of the C-ABI entry point and the symbol table."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ground_filter_common as G
import overviews_common as M
import pcr
import terrain_common as T
from conftest import ROOT, load_cabi

CPU = pcr.ExecutionMode.CPU
P = pcr.TerrainProduct
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (34, 64), (67, 129)]
F32 = np.float32


def all_canonical(a):
    return bool((a.view(np.uint32)[np.isnan(a)] == T.NAN_BITS).all())


# ---- 1: the host loop is the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("nan_fraction", [0.0, 0.3])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_loop_equals_the_model(shape, nan_fraction, edges):
    h, w = shape
    sp = T.spec(compute_edges=edges)
    for src in (T.hills(w, h, 11, nan_fraction), T.values(w, h, 12, nan_fraction)):       # the second: +-Inf, FLT_MAX, denormals, sNaN
        want = T.terrain(src, T.PRODUCTS, edges=edges)
        got = T.host(src, T.PRODUCTS, sp)
        assert got.shape == (7, h, w) and all_canonical(got)
        for k, p in enumerate(T.PRODUCTS):
            T.bits_equal(got[k], want[k], f"all seven: {T.NAMES[k]}")
            T.bits_equal(T.host(src, [p], sp)[0], want[k], f"alone: {T.NAMES[k]}")


def test_parameters_reach_the_arithmetic():
    src = T.hills(40, 30, 13)
    kw = dict(z_factor=2.5, azimuth=120.0, altitude=30.0)
    for cx, cy in ((1.0, -1.0), (0.5, -2.0), (-0.5, 2.0)):
        want = T.terrain(src, T.PRODUCTS, cell_size_x=cx, cell_size_y=cy, **kw)
        got = T.host(src, T.PRODUCTS, T.spec(**kw), cx, cy)
        for k in range(7):
            T.bits_equal(got[k], want[k], f"{cx} {cy} {T.NAMES[k]}")
    assert not (T.host(src, [P.Hillshade], T.spec(**kw))[0] == T.host(src, [P.Hillshade])[0]).all()


def test_one_thread_and_many_give_the_same_bits():
    src = T.values(150, 120, 14, 0.1)
    one, many = T.host(src, T.PRODUCTS, threads=1), T.host(src, T.PRODUCTS, threads=7)
    M.bits_equal(one, many, "threads")


# ---- 2: known answers ------------------------------------------------------------------------------------------------------------
TILTS = [(0, -1, 0.0), (-1, -1, 45.0), (-1, 0, 90.0), (-1, 1, 135.0), (0, 1, 180.0), (1, 1, 225.0), (1, 0, 270.0), (1, -1, 315.0)]


@pytest.mark.parametrize("cx,cy", [(1.0, -1.0), (1.0, 1.0), (-1.0, -1.0), (-2.0, 0.5)])
def test_planes(cx, cy):
    # z = alpha x + beta y falls towards (-alpha, -beta): the aspect is that bearing whichever way rows and columns run
    for a, b, bearing in TILTS:
        alpha, beta = 0.25 * a, 0.25 * b
        z = T.plane(9, 7, alpha, beta, cx, cy, z0=0.0)
        slope, pct, aspect = T.host(z, [P.SlopeDegrees, P.SlopePercent, P.Aspect], None, cx, cy)[:, 1:-1, 1:-1]
        want = math.degrees(math.atan(math.hypot(alpha, beta)))
        assert np.abs(slope.astype(np.float64) - want).max() <= 4 * np.spacing(F32(90.0)), (a, b)
        assert np.abs(pct.astype(np.float64) - 100.0 * math.hypot(alpha, beta)).max() <= 1e-4
        assert (aspect == F32(bearing)).all(), (a, b, aspect[0, 0], bearing)


def test_flat_band():
    z = np.full((6, 8), 123.5, F32)
    sin_alt = pcr.terrain_light()[0]
    out = T.host(z, T.PRODUCTS)[:, 1:-1, 1:-1]
    for k, want in enumerate((0.0, 0.0, -1.0, F32(1.0 + 254.0 * sin_alt), 0.0, 0.0, 0.0)):
        assert (out[k] == F32(want)).all(), T.NAMES[k]
    assert pcr.terrain_light() == pcr.terrain_light(315.0, 45.0)
    assert abs(sin_alt - math.sin(math.radians(45.0))) < 1e-15


def test_a_slope_facing_away_from_a_low_sun_is_1():
    # the light comes from the north-west, 10 degrees up; the surface falls steeply to the south-east
    z = T.plane(9, 9, -1.0, 1.0)
    hs = T.host(z, [P.Hillshade], T.spec(altitude=10.0))[0, 1:-1, 1:-1]
    assert (hs == F32(1.0)).all()
    lit = T.host(T.plane(9, 9, 1.0, -1.0), [P.Hillshade], T.spec(altitude=10.0))[0, 1:-1, 1:-1]
    assert (lit > F32(100.0)).all()


def test_tri_tpi_roughness_known_answer():
    z = np.zeros((3, 3), F32)
    z[1, 1] = 8.0
    tri, tpi, rough = T.host(z, [P.TRI, P.TPI, P.Roughness])[:, 1, 1]
    assert (tri, tpi, rough) == (8.0, 8.0, 8.0)
    z = np.arange(9, dtype=F32).reshape(3, 3)
    tri, tpi, rough = T.host(z, [P.TRI, P.TPI, P.Roughness])[:, 1, 1]
    assert (tri, tpi, rough) == (2.5, 0.0, 8.0)


# ---- 3: atan_deg -------------------------------------------------------------------------------------------------------------------
def ulps_of(err, full_scale):
    return err / float(np.spacing(F32(full_scale)))                    # 2^-17 at 90, 2^-15 at 360


def test_atan_deg_accuracy_slope():
    """Measured: 1.241e-5 degrees = 1.63 ulp of 90 over the sweep; asserted: its whole-ulp ceiling, 2, under the condition 4."""
    rng = np.random.default_rng(2024)
    edge = []
    for t in (T.TAN_PI_8, T.TAN_3PI_8):
        edge += [np.nextafter(t, F32(0)), t, np.nextafter(t, F32(np.inf))]
    x = np.concatenate([
        np.array([0.0, np.inf, 1.0, 1e-45, 1e-40, 1.1754944e-38, 3.4028235e38] + edge, F32),
        rng.uniform(0.0, 4.0, 600_000).astype(F32),
        (2.0 ** rng.uniform(-60.0, 60.0, 600_000)).astype(F32),
    ])
    got = T.atan_deg(x).astype(np.float64)
    want = np.degrees(np.arctan(x.astype(np.float64)))
    err = float(np.abs(got - want).max())
    ulps = ulps_of(err, 90.0)
    print(f"atan_deg, slope: max error {err:.3e} degrees = {ulps:.2f} ulp of 90 over {x.size} arguments")
    assert T.atan_deg(np.array([0.0, np.inf], F32)).tolist() == [0.0, 90.0]
    assert ulps <= 2.0
    assert ulps <= 4.0                                               # the condition: 3.05e-5 degrees


def test_atan_deg_accuracy_aspect():
    """Measured: 2.627e-5 degrees = 0.86 ulp of 360 over the sweep; asserted: its whole-ulp ceiling, 1, under the condition 4."""
    rng = np.random.default_rng(2025)
    n = 1_200_000
    mag = 2.0 ** rng.uniform(-30.0, 30.0, n)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    p, q = mag * np.cos(ang), mag * np.sin(ang) * 2.0 ** rng.uniform(-12.0, 12.0, n)
    axis = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [1.0, 1e-300], [1e-300, -1.0], [-1e-30, -1.0]])
    p, q = np.concatenate([p, axis[:, 0]]), np.concatenate([q, axis[:, 1]])
    with np.errstate(all="ignore"):
        t = T.atan_deg((np.abs(p) / np.abs(q)).astype(F32))
        r = np.where(q <= 0.0, np.where(p > 0.0, F32(360.0) - t, t), np.where(p > 0.0, F32(180.0) + t, F32(180.0) - t)).astype(F32)
    r = np.where(r == F32(360.0), F32(0.0), r).astype(np.float64)
    want = np.degrees(np.arctan2(-p, -q)) % 360.0
    d = np.abs(r - want)
    d = np.minimum(d, 360.0 - d)                                     # 359.99999 and 0 are neighbours
    err = float(d.max())
    ulps = ulps_of(err, 360.0)
    print(f"atan_deg, aspect: max error {err:.3e} degrees = {ulps:.2f} ulp of 360 over {p.size} gradients")
    assert ((r >= 0.0) & (r < 360.0)).all()
    assert ulps <= 1.0
    assert ulps <= 4.0                                               # the condition: 1.22e-4 degrees


# ---- 4: masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(34, 64), (5, 1), (3, 3)])
def test_masks(shape):
    h, w = shape
    src = T.hills(w, h, 15, 0.1)
    nan = np.isnan(src)
    pad = np.ones((h + 2, w + 2), bool)                              # outside the image counts as missing: the 1-cell frame
    pad[1:-1, 1:-1] = nan
    dil = np.zeros((h, w), bool)
    for dr in range(3):
        for dc in range(3):
            dil |= pad[dr:dr + h, dc:dc + w]
    strict, edges = T.host(src, T.PRODUCTS), T.host(src, T.PRODUCTS, T.spec(compute_edges=True))
    for k in range(7):
        assert (np.isnan(strict[k]) == dil).all(), T.NAMES[k]
        assert (np.isnan(edges[k]) == nan).all(), T.NAMES[k]


# ---- 5: pcr.terrain ---------------------------------------------------------------------------------------------------------------
def test_free_function_on_host_grids():
    a, b = T.hills(50, 40, 16, 0.05), T.values(50, 40, 17)
    grid = T.make_grid([a, b])
    sp = T.spec(z_factor=2.0, compute_edges=True, azimuth=200.0, altitude=60.0)
    order = [P.Hillshade, P.TPI, P.SlopeDegrees]
    out = pcr.terrain(grid, 1, order, sp, 2.0, -0.5)
    assert out.location() == pcr.MemoryLocation.Host
    assert [out.band_desc(k).name for k in range(out.num_bands())] == ["hillshade", "tpi", "slope"]
    want = T.terrain(b, order, z_factor=2.0, edges=True, azimuth=200.0, altitude=60.0, cell_size_x=2.0, cell_size_y=-0.5)
    for k, band in enumerate(T.grid_bands(out)):
        T.bits_equal(band, want[k], f"band {k}")
    names = [pcr.terrain(grid, 0, [p]).band_desc(0).name for p in T.PRODUCTS]
    assert names == T.NAMES
    for args, msg in (((grid, 2, [P.TRI]), "band index outside the grid"), ((grid, -1, [P.TRI]), "band index outside the grid"),
                      ((grid, 0, []), "no product asked for"), ((grid, 0, [P.TRI, P.TPI, P.TRI]), "duplicate product tri"),
                      ((grid, 0, [P.TRI], T.spec(z_factor=0.0)), "z_factor must be finite and not zero"),
                      ((grid, 0, [P.TRI], T.spec(z_factor=float("inf"))), "z_factor must be finite and not zero"),
                      ((grid, 0, [P.TRI], T.spec(altitude=91.0)), "altitude must be between 0 and 90"),
                      ((grid, 0, [P.TRI], T.spec(azimuth=float("nan"))), "azimuth must be finite"),
                      ((grid, 0, [P.TRI], None, 0.0, -1.0), "cell sizes must be finite and not zero"),
                      ((grid, 0, [P.TRI], None, 1.0, float("nan")), "cell sizes must be finite and not zero")):
        with pytest.raises(RuntimeError, match=msg):
            pcr.terrain(*args)
    d = pcr.BandDesc()
    d.name, d.dtype = "ids", pcr.DataType.Int32
    with pytest.raises(RuntimeError, match="terrain needs a Float32 band"):
        pcr.terrain(pcr.Grid.create(8, 8, [d]), 0, [P.TRI])


# ---- 6: C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    src = C.c_void_p(0x100000)                                        # never dereferenced: every call is refused first
    nan, inf = float("nan"), float("inf")

    def call(s=src, w=16, h=16, ss=16, n=None, products=(3, 0), dsts=(0x200000, 0x300000), ds=(16, 16), cx=1.0, cy=-1.0, z=1.0,
             edges=0, light=(0.7, -0.5, 0.5), null=()):
        k = len(products) if n is None else n
        pr = None if "products" in null else (C.c_int * max(len(products), 1))(*products)
        dp = None if "dsts" in null else (C.c_void_p * max(len(dsts), 1))(*dsts)
        st = None if "strides" in null else (C.c_int64 * max(len(ds), 1))(*ds)
        return L.pcr_hip_terrain(s, w, h, ss, k, pr, dp, st, cx, cy, z, edges, light[0], light[1], light[2], None)

    last = 4 * (15 * 16 + 15)
    for kw, msg in ((dict(s=None), b"null argument"), (dict(null=("products",)), b"null argument"),
                    (dict(null=("dsts",)), b"null argument"), (dict(null=("strides",)), b"null argument"),
                    (dict(dsts=(0x200000, 0)), b"null argument"),
                    (dict(w=0), b"must be positive"), (dict(h=-1), b"must be positive"),
                    (dict(n=0), b"n_products must be between 1 and 7"), (dict(n=8), b"n_products must be between 1 and 7"),
                    (dict(products=(3, 7)), b"unknown product"), (dict(products=(-1, 2)), b"unknown product"),
                    (dict(products=(3, 3)), b"duplicate product"),
                    (dict(ss=15), b"src_stride smaller than width"), (dict(ds=(16, 15)), b"dst_stride smaller than width"),
                    (dict(cx=0.0), b"cell sizes must be finite and not zero"), (dict(cy=nan), b"cell sizes must be finite and not zero"),
                    (dict(cx=inf), b"cell sizes must be finite and not zero"),
                    (dict(z=0.0), b"z_factor must be finite and not zero"), (dict(z=nan), b"z_factor must be finite and not zero"),
                    (dict(edges=2), b"edges must be 0 or 1"), (dict(edges=-1), b"edges must be 0 or 1"),
                    (dict(light=(nan, 0.0, 0.0)), b"the light constants must be finite"),
                    (dict(dsts=(0x100000, 0x300000)), b"dst overlaps src"),
                    (dict(dsts=(0x200000, 0x100000 + last)), b"dst overlaps src"),
                    (dict(dsts=(0x200000, 0x200000 + last)), b"dst overlaps another dst"),
                    (dict(h=65536 * 32, dsts=(0x40000000, 0x80000000)), b"more than 65535 tile rows")):
        assert call(**kw) == 1, kw
        assert b"terrain: " in L.pcr_hip_last_error() and msg in L.pcr_hip_last_error(), (kw, L.pcr_hip_last_error())
    assert L.pcr_hip_abi_version() == 5


def test_symbol_table_equals_the_header():
    A = load_cabi()
    text = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(pcr_hip_[a-z0-9_]+)\s*\(", text)))
    assert sorted(A.SYMBOLS) == names
    assert "pcr_hip_terrain" in names and hasattr(C.CDLL(A.LIB_PATH), "pcr_hip_terrain")
    ids = dict(re.findall(r"PCR_HIP_TERRAIN_([A-Z_]+) = (\d)", text))
    assert [int(ids[k]) for k in ("SLOPE_DEGREES", "SLOPE_PERCENT", "ASPECT", "HILLSHADE", "TRI", "TPI", "ROUGHNESS")] == \
        [int(p) for p in T.PRODUCTS] == list(range(7))


# ---- 7: the host-engine pipeline -------------------------------------------------------------------------------------------------
W, H, NPTS, RADIUS = 64, 48, 6000, 2


def run_pipeline(cfg, clouds):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "host"
    out = []
    for c in clouds:
        pipe.ingest(c)
        pipe.finalize()
        res = pipe.result()
        out.append(([res.band_desc(b).name for b in range(res.num_bands())], G.grid_bands(res)))
    return out


def terrain_entries():
    return [T.band_cfg("dtm", P.Hillshade), T.band_cfg("dtm", P.SlopeDegrees), T.band_cfg("value_1", P.Roughness, "canopy roughness"),
            T.band_cfg("dtm", P.Aspect, compute_edges=True), T.band_cfg("hag", P.TPI, z_factor=2.0),
            T.band_cfg("dtm", P.Hillshade, "dtm_hillshade_east", azimuth=90.0, altitude=30.0)]


@pytest.fixture(scope="module")
def clouds():
    return G.cloud(W, H, NPTS, seed=81), G.cloud(W, H, NPTS // 4, seed=82)


def test_terrain_is_off_by_default():
    cfg = pcr.PipelineConfig()
    assert list(cfg.terrain) == []
    t = pcr.TerrainBandConfig()
    assert (t.source_band, t.band_name, t.product) == ("", "", P.Hillshade)
    assert (t.z_factor, t.compute_edges, t.azimuth, t.altitude) == (1.0, False, 315.0, 45.0)


@pytest.mark.parametrize("radius", [0, RADIUS])
def test_host_pipeline_bands_order_and_steps(tmp_path, clouds, radius):
    base = run_pipeline(G.pipeline_cfg(W, H, CPU, radius=radius), clouds)
    cfg = G.pipeline_cfg(W, H, CPU, radius=radius)
    cfg.terrain = terrain_entries()
    cfg.output_path = str(tmp_path / "t.tif")
    got = run_pipeline(cfg, clouds)
    new = ["dtm_hillshade", "dtm_slope", "canopy roughness", "dtm_aspect", "hag_tpi", "dtm_hillshade_east"]
    for k in range(2):                                        # (k = 1: a second finalize() after another ingest is right again)
        names, bands = got[k]
        assert names == base[k][0] + new
        for b in range(5):
            M.bits_equal(bands[b], base[k][1][b], f"finalize {k}: band {b} is what it is without the field")
        sources = dict(zip(names[:5], bands[:5]))             # the bands as they leave the pipeline: filled
        want = T.expect_bands(sources, cfg)
        for j, name in enumerate(new):
            T.bits_equal(bands[5 + j], want[j], f"finalize {k}: {name}")
            assert all_canonical(bands[5 + j])
        # ... and the model itself, once: the hillshade of the (filled) DTM, never filled again
        T.bits_equal(bands[5], T.terrain(bands[3], [P.Hillshade])[0], "model")
        if radius:
            assert np.isnan(bands[5]).any(), "terrain bands are not filled"
    assert pcr.read_geotiff_band_names(cfg.output_path) == got[1][0]
    for b, band in enumerate(got[1][1]):
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), band, f"file band {b}")


def test_without_ground_on_an_average_band(clouds):
    cfg = G.pipeline_cfg(W, H, CPU, ground=False, radius=RADIUS)
    r = pcr.ReductionSpec()
    r.value_channel, r.type, r.output_band_name = "value", pcr.ReductionType.Average, "mean"
    cfg.reductions = list(cfg.reductions) + [r]
    cfg.terrain = [T.band_cfg("mean", P.SlopePercent), T.band_cfg("mean", P.TRI, compute_edges=True)]
    names, bands = run_pipeline(cfg, clouds[:1])[0]
    assert names == list(G.BANDS) + ["mean", "mean_slope_percent", "mean_tri"]
    T.bits_equal(bands[4], T.terrain(bands[3], [P.SlopePercent])[0], "slope percent of the filled mean")
    T.bits_equal(bands[5], T.terrain(bands[3], [P.TRI], edges=True)[0], "tri")


def test_overview_levels_carry_the_new_bands(tmp_path):
    Wc, Hc = 520, 512                                          # write_cog's rule gives a level only from 512 cells a side
    cfg = G.pipeline_cfg(Wc, Hc, CPU, radius=2)
    cfg.terrain = [T.band_cfg("dtm", P.Hillshade), T.band_cfg("dtm", P.SlopeDegrees)]
    cfg.output_path, cfg.write_cog = str(tmp_path / "c.tif"), True
    names, bands = run_pipeline(cfg, [G.cloud(Wc, Hc, 200_000, seed=83)])[0]
    assert names[5:] == ["dtm_hillshade", "dtm_slope"]
    assert pcr.read_geotiff_overviews(cfg.output_path) == [(260, 256)]
    for b in range(7):
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), bands[b], f"band {b}")
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), M.down(bands[b]), f"band {b} level 1")


def test_create_errors():
    def refused(entries, **kw):
        cfg = G.pipeline_cfg(W, H, kw.pop("mode", CPU), **kw)
        cfg.terrain = entries
        assert pcr.Pipeline.create(cfg) is None
        return pcr.pipeline_create_error()
    ok = T.band_cfg("dtm", P.Hillshade)
    assert refused([ok, T.band_cfg("z_2", P.TRI)]) == "pipeline: terrain[1].source_band 'z_2' names no band of the result"
    assert refused([T.band_cfg("", P.TRI)]) == "pipeline: terrain[0].source_band '' names no band of the result"
    assert refused([T.band_cfg("dtm", P.TRI)], ground=False) == "pipeline: terrain[0].source_band 'dtm' names no band of the result"
    assert refused([T.band_cfg("hag", P.TRI)], top=False) == "pipeline: terrain[0].source_band 'hag' names no band of the result"
    # a terrain band is no source
    assert refused([ok, T.band_cfg("dtm_hillshade", P.TRI)]) == \
        "pipeline: terrain[1].source_band 'dtm_hillshade' names no band of the result"
    assert refused([T.band_cfg("dtm", P.TRI, "value_5")]) == "pipeline: terrain[0].band_name 'value_5' clashes with another band"
    assert refused([T.band_cfg("dtm", P.TRI, "hag")]) == "pipeline: terrain[0].band_name 'hag' clashes with another band"
    assert refused([ok, ok]) == "pipeline: terrain[1].band_name 'dtm_hillshade' clashes with another band"
    assert refused([T.band_cfg("dtm", P.TRI, z_factor=0.0)]) == "pipeline: terrain[0].z_factor must be finite and not zero"
    assert refused([ok, T.band_cfg("dtm", P.TRI, altitude=-1.0)]) == "pipeline: terrain[1].altitude must be between 0 and 90"
    assert refused([T.band_cfg("dtm", P.TRI, azimuth=float("inf"))]) == "pipeline: terrain[0].azimuth must be finite"
    for mode in (CPU, pcr.ExecutionMode.GPU):
        cfg = G.pipeline_cfg(W, H, mode, ground=False)
        cfg.terrain = [T.band_cfg("value_2", P.Hillshade)]
        cfg.shard_row_begin, cfg.shard_row_end = 16, 32
        assert pcr.Pipeline.create(cfg) is None
        assert pcr.pipeline_create_error() == "pipeline: terrain bands need the whole grid; derive them from the gathered grid with terrain"


def test_gathered_grid_of_a_sharded_run_is_finished_like_the_unsharded_result(clouds):
    # what rank 0 of a ShardedPipeline does to the grid it gathered (both the C++ class and pcr.distributed call this)
    from pcr import _pcr
    raw = run_pipeline(G.pipeline_cfg(W, H, CPU, ground=False), clouds[:1])[0][1]
    for ground in (True, False):
        cfg = G.pipeline_cfg(W, H, CPU, ground=ground, radius=RADIUS)
        cfg.terrain = terrain_entries() if ground else [T.band_cfg("value_2", P.Hillshade), T.band_cfg("value_1", P.Roughness)]
        names, bands = run_pipeline(cfg, clouds[:1])[0]
        whole = _pcr._finish_gathered(G.make_grid(raw, list(G.BANDS)), cfg)
        assert [whole.band_desc(b).name for b in range(whole.num_bands())] == names
        for b, band in enumerate(G.grid_bands(whole)):
            M.bits_equal(band, bands[b], f"band {b}")
    cfg.terrain = [T.band_cfg("nope", P.TRI)]
    with pytest.raises(RuntimeError, match="names no band of the result"):
        _pcr._check_terrain(cfg)
