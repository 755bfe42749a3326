"""The ground filter without a GPU: a known answer that needs no implementation, the host loop against the NumPy model of the
contract (tests/ground_filter_common.py) bit for bit, special values, the thread count, the argument errors of the three C-ABI
entry points, the host-engine pipeline's PipelineConfig.ground (order of the steps, GeoTIFF, overview level, second finalize),
the create errors, and the host loop under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ground_filter_common as G
import overviews_common as M
import pcr
from conftest import ROOT, load_cabi

PKG = os.path.join(ROOT, "pointcloud-raster_amd")
CPU = pcr.ExecutionMode.CPU


def host_filter(a, spec=None, cell=1.0):
    out = pcr.ground_filter(G.make_grid([a]), 0, spec, cell)
    assert out.num_bands() == 1 and out.band_desc(0).name == "dtm" and out.location() == pcr.MemoryLocation.Host
    return G.grid_bands(out)[0]


# ---- 1: a known answer ---------------------------------------------------------------------------------------------------------
def known_scene():
    yy, xx = np.mgrid[0:48, 0:64]
    z = (10 + 0.01 * xx + 0.02 * yy).astype(np.float32)
    box = np.zeros((48, 64), bool)
    box[20:29, 30:39] = True
    z[box] += np.float32(5)
    empty = np.random.default_rng(1).random((48, 64)) < 0.2
    z[empty] = np.nan
    return z, box, empty


def test_known_answer():
    z, box, empty = known_scene()
    radii, thresholds = G.levels()
    assert radii == [1, 2, 4, 8, 16]
    assert [float(t) for t in thresholds] == [float(np.float32(x)) for x in (0.15, 2.15, 2.5, 2.5, 2.5)]
    got_r, got_t = pcr.ground_filter_levels(pcr.GroundFilterSpec(), 1.0)
    assert got_r == radii and [np.float32(t) for t in got_t] == thresholds
    for name, dtm in (("model", G.ground_filter(z, radii, thresholds)), ("host", host_filter(z))):
        assert (np.isnan(dtm) == (box | empty)).all(), f"{name}: the DTM is NaN exactly on the box and on the empty cells"
        keep = ~np.isnan(dtm)
        M.bits_equal(dtm[keep], z[keep], f"{name}: every other cell keeps its source bits")
        assert (dtm.view(np.uint32)[~keep] == 0x7FC00000).all(), name


def test_defaults_are_pdals():
    s = pcr.GroundFilterSpec()
    assert (s.max_radius_cells, s.exponential, s.slope) == (16, True, 1.0)
    assert (np.float32(s.initial_distance), np.float32(s.max_distance)) == (np.float32(0.15), np.float32(2.5))


@pytest.mark.parametrize("cell", [1.0, 0.5, 0.3, 2.0])
@pytest.mark.parametrize("exponential", [True, False])
def test_schedule_equals_the_model(exponential, cell):
    for kw in (dict(), dict(max_radius_cells=64), dict(max_radius_cells=1), dict(slope=0.37, initial_distance=0.1, max_distance=7.3),
               dict(slope=0.0), dict(max_radius_cells=3, initial_distance=2.5)):
        kw = dict(kw, exponential=exponential)
        radii, thresholds = pcr.ground_filter_levels(G.spec(**kw), cell)
        want_r, want_t = G.levels(cell=cell, **kw)
        assert radii == want_r
        assert np.array(thresholds, np.float32).tobytes() == np.array(want_t, np.float32).tobytes(), (kw, cell)
        assert all(b > a for a, b in zip(radii, radii[1:])) and radii[0] == 1 and radii[-1] <= kw.get("max_radius_cells", 16)


def test_spec_errors():
    g = G.make_grid([np.zeros((4, 4), np.float32)])
    for kw, msg in ((dict(max_radius_cells=0), "max_radius_cells must be between 1 and 64"),
                    (dict(max_radius_cells=65), "max_radius_cells must be between 1 and 64"),
                    (dict(slope=-1.0), "slope must be finite"), (dict(slope=float("nan")), "slope must be finite"),
                    (dict(initial_distance=float("inf")), "initial_distance must be finite"),
                    (dict(max_distance=0.1), "max_distance must be finite and not below initial_distance")):
        with pytest.raises(RuntimeError, match=msg):
            pcr.ground_filter(g, 0, G.spec(**kw))
        with pytest.raises(RuntimeError, match=msg):
            pcr.ground_filter_levels(G.spec(**kw), 1.0)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="cell_size must be finite and positive"):
            pcr.ground_filter(g, 0, None, cell)
    for band, top in ((1, None), (-1, None), (0, 1)):
        with pytest.raises(RuntimeError, match="band index outside the grid"):
            pcr.ground_filter(g, band, None, 1.0, top)


# ---- 2: the host loop equals the model ----------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 40), (40, 1), (7, 5), (45, 67), (70, 130)]                     # (rows, cols)
SCHEDULES = [(True, 1), (True, 3), (True, 16), (True, 64), (False, 1), (False, 3), (False, 16)]


@pytest.mark.parametrize("nan_fraction", [0.0, 0.2, 0.9, 1.0])
@pytest.mark.parametrize("schedule", SCHEDULES, ids=lambda s: ("exp" if s[0] else "lin") + str(s[1]))
@pytest.mark.parametrize("shape", SHAPES)
def test_host_loop_equals_the_model(shape, schedule, nan_fraction):
    h, w = shape
    exponential, max_radius = schedule
    a = G.terrain(w, h, seed=w * 1000 + h + max_radius, nan_fraction=nan_fraction)
    kw = dict(exponential=exponential, max_radius_cells=max_radius)
    got = host_filter(a, G.spec(**kw))
    G.bits_equal(got, G.ground_filter(a, *G.levels(**kw)), f"{h}x{w} {kw} nan={nan_fraction}")
    keep = ~np.isnan(got)
    M.bits_equal(got[keep], a[keep], "ground cells keep their source bits")
    assert (got.view(np.uint32)[~keep] == 0x7FC00000).all()
    if nan_fraction == 1.0:
        assert not keep.any()


@pytest.mark.parametrize("R", [1, 2, 5, 31, 32, 64])
def test_single_levels_and_the_mixed_values_equal_the_model(R):
    # every radius on its own (the schedules above always start at 1), on values of every kind: +-Inf, FLT_MAX, -0.0,
    # denormals, NaNs of several payloads
    from pcr import _pcr
    for a in (G.terrain(67, 45, seed=R, nan_fraction=0.2), M.values(67, 45, seed=R, nan_fraction=0.2)):
        got = _pcr._ground_filter_host(a, [R], [0.5])
        G.bits_equal(got, G.ground_filter(a, [R], [np.float32(0.5)]), f"R={R}")


# ---- 3: special values ------------------------------------------------------------------------------------------------------------
def test_inf_cells_stay_ground_where_the_difference_is_nan():
    a = np.full((9, 9), 1.0, np.float32)
    a[4, 4] = np.inf                                          # opening with R = 1 leaves 1 there: Inf - 1 = Inf > t, non-ground
    b = np.full((9, 9), np.inf, np.float32)                   # Inf - Inf = NaN compares false: ground
    c = np.full((9, 9), -np.inf, np.float32)
    c[4, 4] = 0.0                                             # 0 - -Inf = Inf: non-ground
    for x in (a, b, c):
        G.bits_equal(host_filter(x), G.ground_filter(x, *G.levels()), "model")
    assert np.isnan(host_filter(a)[4, 4]) and not np.isnan(host_filter(a)[0, 0])
    M.bits_equal(host_filter(b), b, "Inf - Inf leaves every cell ground")
    got = host_filter(c)
    assert np.isnan(got[4, 4]) and (got[np.arange(81).reshape(9, 9) != 40] == -np.inf).all()


def test_negative_zero_survives():
    a = np.zeros((12, 12), np.float32)
    a[::2, ::3] = np.float32(-0.0)
    a[5, 5] = np.nan
    got = host_filter(a)
    want = a.copy()
    want.view(np.uint32)[5, 5] = 0x7FC00000
    M.bits_equal(got, want, "-0.0 and +0.0 are equal to the filter and keep their bits")


def test_threshold_capped_by_max_distance_and_slope_zero():
    # a 3 x 3 block 2 above the plain survives R = 1 (it is wider than the window) and meets R = 2 with t2:
    #   default slope: t2 = 0.15 + 1 * 1 * 2 * 1 = 2.15 -- stays;  max_distance = 1.9 caps it -- goes;  slope = 0: t2 = 0.15 -- goes
    a = np.zeros((15, 15), np.float32)
    a[6:9, 6:9] = 2.0
    block = a > 0
    for kw, goes in ((dict(max_radius_cells=2), False), (dict(max_radius_cells=2, max_distance=1.9), True),
                     (dict(max_radius_cells=2, slope=0.0), True)):
        radii, thresholds = pcr.ground_filter_levels(G.spec(**kw), 1.0)
        assert radii == [1, 2]
        got = host_filter(a, G.spec(**kw))
        G.bits_equal(got, G.ground_filter(a, *G.levels(**kw)), str(kw))
        assert (np.isnan(got) == (block if goes else np.zeros_like(block))).all(), kw
    assert pcr.ground_filter_levels(G.spec(max_distance=1.9), 1.0)[1][1:] == [np.float32(1.9)] * 4
    assert pcr.ground_filter_levels(G.spec(slope=0.0), 1.0)[1] == [np.float32(0.15)] * 5


def test_hag_band():
    a = G.terrain(60, 40, seed=3)
    top = (a + np.float32(2.0)).astype(np.float32)
    top[3, 3] = np.nan
    out = pcr.ground_filter(G.make_grid([top, a]), 1, None, 1.0, 0)
    assert [out.band_desc(b).name for b in range(out.num_bands())] == ["dtm", "hag"]
    dtm, hag = G.grid_bands(out)
    M.bits_equal(dtm, host_filter(a), "dtm")
    M.bits_equal(hag, G.difference(top, dtm), "hag = top - dtm, NaN (0x7FC00000) where either is")
    assert np.isnan(hag[3, 3])


# ---- 4: thread counts -----------------------------------------------------------------------------------------------------------
THREADS_SCRIPT = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import ground_filter_common as G
import pcr
a = G.terrain(150, 120, seed=9, nan_fraction=0.3)
out = G.grid_bands(pcr.ground_filter(G.make_grid([a]), 0, G.spec(max_radius_cells=8)))[0]
sys.stdout.write(out.tobytes().hex())
"""


def test_thread_count_does_not_change_the_bits():
    paths = [os.path.join(ROOT, "tests"), os.path.dirname(os.path.dirname(pcr.__file__))]
    runs = []
    for n in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=n)
        out = subprocess.run([sys.executable, "-c", THREADS_SCRIPT.format(paths=paths)], capture_output=True, text=True, env=env,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        runs.append(out.stdout)
    assert len(runs[0]) == 150 * 120 * 8 and runs[0] == runs[1]


# ---- 5: C-ABI -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    src, dst, work = C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_void_p(0x300000)   # never dereferenced: every call is refused first
    need = C.c_size_t(0)
    assert L.pcr_hip_ground_filter_work_bytes(16, 16, C.byref(need)) == 0               # answers without a device
    assert need.value >= 3 * 16 * 16 * 4
    assert L.pcr_hip_ground_filter_work_bytes(0, 16, C.byref(need)) == 1 and b"must be positive" in L.pcr_hip_last_error()
    assert L.pcr_hip_ground_filter_work_bytes(16, 16, None) == 1 and b"null argument" in L.pcr_hip_last_error()
    L.pcr_hip_ground_filter_work_bytes(16, 16, C.byref(need))
    nan, inf = float("nan"), float("inf")

    def call(s=src, d=dst, w=16, h=16, ss=16, ds=16, levels=None, radii=(1, 2), thr=(0.5, 0.5), wk=work, wb=None,
             null_radii=False, null_thr=False):
        n = len(radii) if levels is None else levels
        rad = None if null_radii else (C.c_int * max(len(radii), 1))(*radii)
        th = None if null_thr else (C.c_float * max(len(thr), 1))(*thr)
        return L.pcr_hip_ground_filter(s, d, w, h, ss, ds, n, rad, th, wk, need.value if wb is None else wb, None)

    for kw, msg in ((dict(s=None), b"null argument"), (dict(d=None), b"null argument"), (dict(wk=None), b"null argument"),
                    (dict(null_radii=True), b"null argument"), (dict(null_thr=True), b"null argument"),
                    (dict(w=0), b"must be positive"), (dict(h=-1), b"must be positive"),
                    (dict(ss=15), b"src_stride smaller than width"), (dict(ds=15), b"dst_stride smaller than width"),
                    (dict(levels=0), b"levels must be between 1 and 64"),
                    (dict(radii=tuple(range(1, 66)), thr=(0.5,) * 65), b"levels must be between 1 and 64"),
                    (dict(radii=(0, 2)), b"a radius must be between 1 and 64"), (dict(radii=(1, 65)), b"a radius must be between 1 and 64"),
                    (dict(radii=(2, 2)), b"radii must be strictly increasing"), (dict(radii=(3, 2)), b"radii must be strictly increasing"),
                    (dict(thr=(0.5, nan)), b"a threshold must be finite and not negative"),
                    (dict(thr=(inf, 0.5)), b"a threshold must be finite and not negative"),
                    (dict(thr=(0.5, -0.25)), b"a threshold must be finite and not negative"),
                    (dict(wb=need.value - 1), b"work_bytes too small"),
                    (dict(d=src), b"dst overlaps src"),
                    (dict(d=C.c_void_p(0x100000 + 4 * (15 * 16 + 15))), b"dst overlaps src"),       # the last cell of src
                    (dict(wk=C.c_void_p(0x100000 - need.value + 4)), b"the workspace overlaps src"),
                    (dict(wk=C.c_void_p(0x100000 + 4 * 255)), b"the workspace overlaps src"),
                    (dict(wk=C.c_void_p(0x200000 + 4 * 255)), b"the workspace overlaps dst")):
        assert call(**kw) == 1, kw
        assert msg in L.pcr_hip_last_error(), (kw, L.pcr_hip_last_error())

    def diff(t=src, g=dst, d=work, w=16, h=16, ts=16, gs=16, ds=16):
        return L.pcr_hip_band_difference(t, g, d, w, h, ts, gs, ds, None)
    for kw, msg in ((dict(t=None), b"null argument"), (dict(g=None), b"null argument"), (dict(d=None), b"null argument"),
                    (dict(w=0), b"must be positive"), (dict(h=0), b"must be positive"),
                    (dict(ts=15), b"top_stride smaller than width"), (dict(gs=15), b"ground_stride smaller than width"),
                    (dict(ds=15), b"dst_stride smaller than width")):
        assert diff(**kw) == 1, kw
        assert msg in L.pcr_hip_last_error(), (kw, L.pcr_hip_last_error())
    assert L.pcr_hip_abi_version() == 5


def test_symbol_table_equals_the_header():
    A = load_cabi()
    text = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(pcr_hip_[a-z0-9_]+)\s*\(", text)))
    assert sorted(A.SYMBOLS) == names
    lib = C.CDLL(A.LIB_PATH)
    for name in ("pcr_hip_ground_filter_work_bytes", "pcr_hip_ground_filter", "pcr_hip_band_difference"):
        assert name in names and hasattr(lib, name)


# ---- 6: the host-engine pipeline ---------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def host_case():
    c1, c2 = G.cloud(W, H, NPTS, seed=71), G.cloud(W, H, NPTS // 4, seed=72)
    raw = run_pipeline(G.pipeline_cfg(W, H, CPU, ground=False), [c1, c2])
    assert raw[0][0] == list(G.BANDS)
    assert np.isnan(raw[0][1][0]).any() and not np.isnan(raw[0][1][0]).all()
    return c1, c2, raw


def test_ground_is_off_by_default_and_changes_nothing(host_case):
    c1, c2, raw = host_case
    cfg = pcr.PipelineConfig()
    assert cfg.ground.source_band == "" and cfg.ground.top_band == ""
    assert (cfg.ground.dtm_band_name, cfg.ground.hag_band_name, cfg.ground.max_radius_cells) == ("dtm", "hag", 16)
    again = run_pipeline(G.pipeline_cfg(W, H, CPU, ground=False), [c1, c2])
    for k in range(2):
        assert again[k][0] == raw[k][0]
        for b in range(3):
            M.bits_equal(again[k][1][b], raw[k][1][b], f"finalize {k} band {b}")


@pytest.mark.parametrize("radius", [0, RADIUS])
@pytest.mark.parametrize("top", [True, False])
def test_host_pipeline_bands_order_and_steps(tmp_path, host_case, top, radius):
    c1, c2, raw = host_case
    cfg = G.pipeline_cfg(W, H, CPU, top=top, radius=radius)
    cfg.output_path = str(tmp_path / "g.tif")
    got = run_pipeline(cfg, [c1, c2])
    for k in range(2):                                        # (k = 1: a second finalize() after another ingest is right again)
        names, bands = got[k]
        assert names == list(G.BANDS) + ["dtm"] + (["hag"] if top else [])
        rb = raw[k][1]
        # the steps, spelled out: the filter reads the RAW Min band; the DTM is filled like a Min band; hag is the difference
        # of the bands as returned
        dtm = G.grid_bands(pcr.ground_filter(G.make_grid(rb), 0, cfg.ground, 1.0))[0]
        assert np.isnan(dtm).sum() > np.isnan(rb[0]).sum()                   # the filter removed cells
        if radius:
            filled = G.grid_bands(pcr.fill_nodata(G.make_grid(rb + [dtm]), radius, [0, 1, 3]))
            dtm = filled[3]
            for b in (0, 1):
                M.bits_equal(bands[b], filled[b], f"finalize {k}: band {b} is filled")
            assert np.isnan(dtm).sum() < np.isnan(G.grid_bands(pcr.ground_filter(G.make_grid(rb), 0, cfg.ground, 1.0))[0]).sum()
        else:
            for b in (0, 1):
                M.bits_equal(bands[b], rb[b], f"finalize {k}: band {b} is untouched")
        M.bits_equal(bands[2], rb[2], "Count is untouched")
        M.bits_equal(bands[3], dtm, f"finalize {k}: dtm")
        if top:
            M.bits_equal(bands[4], G.difference(bands[1], bands[3]), f"finalize {k}: hag is the difference of the bands as returned")
        want = G.expect(rb, cfg)
        for b in range(len(want)):
            M.bits_equal(bands[b], want[b], f"finalize {k}: band {b} (expect)")
    assert pcr.read_geotiff_band_names(cfg.output_path) == got[1][0]
    for b, band in enumerate(got[1][1]):
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), band, f"file band {b}")


def test_band_names_and_spec_fields_are_honoured(host_case):
    c1, _, raw = host_case
    cfg = G.pipeline_cfg(W, H, CPU, exponential=False, max_radius_cells=5, slope=0.5, dtm_band_name="bare earth",
                         hag_band_name="canopy")
    names, bands = run_pipeline(cfg, [c1])[0]
    assert names == list(G.BANDS) + ["bare earth", "canopy"]
    spec = G.spec(exponential=False, max_radius_cells=5, slope=0.5)
    M.bits_equal(bands[3], G.grid_bands(pcr.ground_filter(G.make_grid(raw[0][1]), 0, spec, 1.0))[0], "dtm")
    G.bits_equal(bands[3], G.ground_filter(raw[0][1][0], *G.levels(exponential=False, max_radius_cells=5, slope=0.5)), "model")


def test_cell_size_is_the_larger_of_the_two(host_case):
    cfg = G.pipeline_cfg(32, 48, CPU)
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, 16.0, 12.0)
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 0.5, -0.25
    cfg.grid.compute_dimensions()
    assert (cfg.grid.width, cfg.grid.height) == (32, 48)
    rng = np.random.default_rng(5)
    c = pcr.PointCloud.create(4000)
    c.set_x_array(rng.uniform(0, 16, 4000))
    c.set_y_array(rng.uniform(0, 12, 4000))
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", rng.normal(10.0, 1.0, 4000).astype(np.float32))
    _, bands = run_pipeline(cfg, [c])[0]
    M.bits_equal(bands[3], G.grid_bands(pcr.ground_filter(G.make_grid(bands[:1]), 0, cfg.ground, 0.5))[0], "cell = 0.5")


def test_overview_level_is_made_from_the_returned_dtm(tmp_path):
    Wc, Hc = 520, 512                                          # write_cog's rule gives a level only from 512 cells a side
    pts = G.cloud(Wc, Hc, 200_000, seed=73)
    cfg = G.pipeline_cfg(Wc, Hc, CPU, radius=2)
    cfg.output_path, cfg.write_cog = str(tmp_path / "c.tif"), True
    names, bands = run_pipeline(cfg, [pts])[0]
    assert pcr.read_geotiff_overviews(cfg.output_path) == [(260, 256)]
    assert np.isnan(bands[3]).any() and not np.isnan(bands[3]).all()
    for b in range(5):
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), bands[b], f"band {b}")
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), M.down(bands[b]), f"band {b} level 1")


def test_create_errors():
    def refused(cfg):
        assert pcr.Pipeline.create(cfg) is None
        return pcr.pipeline_create_error()
    cfg = G.pipeline_cfg(W, H, CPU)
    cfg.ground.source_band = "z_2"
    assert refused(cfg) == "pipeline: ground.source_band 'z_2' names no output band"
    cfg = G.pipeline_cfg(W, H, CPU)
    cfg.ground.top_band = "value_3"
    assert refused(cfg) == "pipeline: ground.top_band 'value_3' names no output band"
    cfg = G.pipeline_cfg(W, H, CPU, dtm_band_name="value_5")
    assert refused(cfg) == "pipeline: ground.dtm_band_name 'value_5' clashes with an output band"
    cfg = G.pipeline_cfg(W, H, CPU, hag_band_name="dtm")
    assert refused(cfg) == "pipeline: ground.hag_band_name 'dtm' clashes with an output band"
    cfg = G.pipeline_cfg(W, H, CPU, max_radius_cells=65)
    assert refused(cfg) == "pipeline: ground.max_radius_cells must be between 1 and 64"
    cfg = G.pipeline_cfg(W, H, CPU, max_distance=0.1)
    assert refused(cfg) == "pipeline: ground.max_distance must be finite and not below initial_distance"
    for mode in (CPU, pcr.ExecutionMode.GPU):
        cfg = G.pipeline_cfg(W, H, mode)
        cfg.shard_row_begin, cfg.shard_row_end = 16, 32
        assert refused(cfg) == "pipeline: ground filter needs the whole grid; filter the gathered grid with ground_filter"
    # a hag name is not looked at when no hag band is asked for
    cfg = G.pipeline_cfg(W, H, CPU, top=False, hag_band_name="dtm")
    assert pcr.Pipeline.create(cfg) is not None, pcr.pipeline_create_error()


def test_gathered_grid_of_a_sharded_run_is_finished_like_the_unsharded_result(host_case):
    # what rank 0 of a ShardedPipeline does to the grid it gathered (both the C++ class and pcr.distributed call this)
    from pcr import _pcr
    c1, _, raw = host_case
    cfg = G.pipeline_cfg(W, H, CPU, radius=RADIUS)
    names, bands = run_pipeline(cfg, [c1])[0]
    whole = _pcr._finish_gathered(G.make_grid(raw[0][1], list(G.BANDS)), cfg)
    assert [whole.band_desc(b).name for b in range(whole.num_bands())] == names
    for b, band in enumerate(G.grid_bands(whole)):
        M.bits_equal(band, bands[b], f"band {b}")
    cfg.ground.source_band = "nope"
    with pytest.raises(RuntimeError, match="names no output band"):
        _pcr._check_ground(cfg)


# ---- 7: sanitizers (the host loop alone, in a program of its own) -------------------------------------------------------------
def test_host_loop_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    host = os.path.join(PKG, "host")
    exe = str(tmp_path / "ground_filter_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=undefined,float-cast-overflow", "-fno-omit-frame-pointer",
                    "-I", os.path.join(host, "include"), "-I", os.path.join(host, "src"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "ground_filter_san.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", OMP_NUM_THREADS="4")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "host ground filter survived" in out.stdout
