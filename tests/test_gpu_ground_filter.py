"""The ground filter on the MI355X: pcr_hip_ground_filter (row and column passes, aprons wider than the image and across several
tiles, rows on 16 bytes and not) and pcr_hip_band_difference through the C-ABI and behind pcr.ground_filter on Device grids, and
the HIP engine's PipelineConfig.ground.  Everything BIT FOR BIT against the host loop, which tests/test_ground_filter.py holds to
the NumPy model of the contract."""
import ctypes as C

import numpy as np
import pytest

import ground_filter_common as G
import overviews_common as M
import pcr
from conftest import load_cabi
from pcr import _pcr

pytestmark = pytest.mark.gpu

# (rows, cols): the smallest; one row, one column; one below, on and one above a 64-wide tile (rows that start on 16 bytes and
# rows that do not); several tiles with ragged edges both ways
SHAPES = [(1, 1), (1, 300), (300, 1), (33, 63), (34, 64), (35, 65), (67, 129), (70, 130), (130, 300)]
# The kernels have no radius classes (LDS is sized by R itself); what changes with R is the apron's padding to whole quads
# (R % 4: 1..5), whether a 64-cell line holds several segments of 2R + 1 cells or one (31 | 32), and the apron against the
# tile and the image (8..64).
RADII = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 64]
SENTINEL = np.float32(-12345.5)


def device_filter(a, radii, thresholds, offset=0, stride=None, work_shift=64):
    """pcr_hip_ground_filter on `a` as a window at float `offset` of a plane with rows `stride` floats apart; dst is a window
    of a plane of sentinels, the workspace sits between guard words.  Returns the window of dst; asserts the guards."""
    A = load_cabi()
    L = A.lib()
    h, w = a.shape
    stride = stride or w
    n = offset + (h - 1) * stride + w + 3
    plane = np.full(n, SENTINEL, np.float32)
    inside = np.zeros(n, bool)
    idx = offset + np.arange(h)[:, None] * stride + np.arange(w)[None, :]
    plane[idx] = a
    plane.view(np.uint32)[idx] = a.view(np.uint32)
    inside[idx] = True
    src = A.DeviceBuffer.from_numpy(plane)
    dst = A.DeviceBuffer.from_numpy(np.full(n, SENTINEL, np.float32))
    bytes_ = C.c_size_t(0)
    A.check(L.pcr_hip_ground_filter_work_bytes(w, h, C.byref(bytes_)))
    guard = np.full((bytes_.value + 2 * work_shift + 3) // 4, SENTINEL, np.float32)
    work = A.DeviceBuffer.from_numpy(guard)
    rad = (C.c_int * len(radii))(*radii)
    thr = (C.c_float * len(radii))(*[float(t) for t in thresholds])
    A.check(L.pcr_hip_ground_filter(C.c_void_p(src.ptr.value + 4 * offset), C.c_void_p(dst.ptr.value + 4 * offset), w, h, stride,
                                    stride, len(radii), rad, thr, C.c_void_p(work.ptr.value + work_shift), bytes_.value, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = dst.to_numpy()
    assert (got[~inside] == SENTINEL).all(), "a store outside dst's window"
    wk = work.to_numpy().view(np.uint8)
    sent = guard.view(np.uint8)
    assert (wk[:work_shift] == sent[:work_shift]).all(), "a store in front of the workspace"
    assert (wk[work_shift + bytes_.value:] == sent[work_shift + bytes_.value:]).all(), "a store behind the workspace"
    M.bits_equal(src.to_numpy(), plane, "the source is only read")
    return got[idx]


def check_device(a, radii, thresholds, what, **kw):
    want = _pcr._ground_filter_host(a, list(radii), [float(t) for t in thresholds])
    got = device_filter(a, radii, thresholds, **kw)
    G.bits_equal(got, want, what)
    keep = ~np.isnan(got)
    M.bits_equal(got[keep], a[keep], "ground cells keep their source bits")
    assert (got.view(np.uint32)[~keep] == 0x7FC00000).all(), "every other cell is the one NaN"
    return got


@pytest.mark.parametrize("nan_fraction", [0.0, 0.3])
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_single_level_equals_the_host_loop(shape, R, nan_fraction):
    h, w = shape
    a = G.terrain(w, h, seed=w * 1000 + h + R, nan_fraction=nan_fraction)
    check_device(a, [R], [0.5], f"{h}x{w} R={R} nan={nan_fraction}")


@pytest.mark.parametrize("nan_fraction", [0.0, 0.3])
@pytest.mark.parametrize("R", [1, 7, 32, 64])
def test_special_values_single_level(R, nan_fraction):
    # +-Inf, FLT_MAX, -0.0, denormals and NaNs of several payloads (a signalling one among them)
    a = M.values(129, 67, seed=R, nan_fraction=nan_fraction)
    check_device(a, [R], [0.5], f"values R={R} nan={nan_fraction}")


@pytest.mark.parametrize("name", ["default", "linear to 64"])
def test_whole_schedules(name):
    spec = G.spec() if name == "default" else G.spec(exponential=False, max_radius_cells=64)
    radii, thresholds = pcr.ground_filter_levels(spec, 1.0)
    assert len(radii) == (5 if name == "default" else 64)
    for seed, a in enumerate((G.terrain(129, 67, seed=5), M.values(129, 67, seed=6, nan_fraction=0.2))):
        got = check_device(a, radii, thresholds, f"{name} schedule, case {seed}")
        assert 0 < np.isnan(got).sum() - np.isnan(a).sum() < a.size            # the filter removed something, not everything
        # and behind pcr.ground_filter on a Device grid, with the hag band
        with np.errstate(invalid="ignore"):                                      # (a signalling NaN among the values)
            top = a + np.float32(1.5)
        g = G.make_grid([a, top])
        host = G.grid_bands(pcr.ground_filter(g, 0, spec, 1.0, 1))
        dev_grid = pcr.ground_filter(g.to(pcr.MemoryLocation.Device), 0, spec, 1.0, 1)
        assert dev_grid.location() == pcr.MemoryLocation.Device
        assert [dev_grid.band_desc(b).name for b in range(dev_grid.num_bands())] == ["dtm", "hag"]
        dev = G.grid_bands(dev_grid.to_host())
        for b in range(2):
            G.bits_equal(dev[b], host[b], f"{name} schedule, Device grid band {b}")
            assert (dev[b].view(np.uint32)[np.isnan(dev[b])] == 0x7FC00000).all()


def test_degenerate_bands():
    radii, thresholds = pcr.ground_filter_levels(G.spec(), 1.0)
    nan = np.full((70, 130), np.nan, np.float32)
    got = check_device(nan, radii, thresholds, "all NaN")
    assert np.isnan(got).all()
    flat = np.full((70, 130), 3.25, np.float32)
    got = check_device(flat, radii, thresholds, "no NaN, flat")
    M.bits_equal(got, flat, "a flat band is all ground")


@pytest.mark.parametrize("R", [5, 64])
@pytest.mark.parametrize("offset", [1, 4])                      # an odd float offset: the scalar accesses; 4: 16-byte rows, stride 520
def test_cabi_window_in_a_strided_plane_and_guard_words(offset, R):
    a = G.terrain(200, 136, seed=91 + offset + R, nan_fraction=0.3)
    stride = 517 if offset == 1 else 520
    check_device(a, [R], [0.5], f"offset {offset} R={R}", offset=offset, stride=stride, work_shift=64 if offset == 4 else 68)
    radii, thresholds = pcr.ground_filter_levels(G.spec(), 1.0)
    check_device(a, radii, thresholds, f"offset {offset}, default schedule", offset=offset, stride=stride)


def test_band_difference():
    A = load_cabi()
    L = A.lib()
    h, w, offset, stride = 35, 65, 1, 71
    top = M.values(w, h, seed=3, nan_fraction=0.2)
    gnd = M.values(w, h, seed=4, nan_fraction=0.2)
    gnd[5, :10] = top[5, :10]                                                 # Inf - Inf where both are Inf, x - x = +0
    want = G.difference(top, gnd)
    n = offset + h * stride
    idx = offset + np.arange(h)[:, None] * stride + np.arange(w)[None, :]
    planes = []
    for a in (top, gnd):
        p = np.full(n, SENTINEL, np.float32)
        p.view(np.uint32)[idx] = a.view(np.uint32)
        planes.append(A.DeviceBuffer.from_numpy(p))
    out = A.DeviceBuffer.from_numpy(np.full(n, SENTINEL, np.float32))
    at = lambda b: C.c_void_p(b.ptr.value + 4 * offset)
    A.check(L.pcr_hip_band_difference(at(planes[0]), at(planes[1]), at(out), w, h, stride, stride, stride, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = out.to_numpy()
    M.bits_equal(got[idx], want, "top - ground, NaN as 0x7FC00000")
    mask = np.zeros(n, bool)
    mask[idx] = True
    assert (got[~mask] == SENTINEL).all()
    # 16-byte rows: the vector variant
    dense = [A.DeviceBuffer.from_numpy(np.ascontiguousarray(x[:, :64])) for x in (top, gnd)]
    out = A.DeviceBuffer(h * 64 * 4)
    A.check(L.pcr_hip_band_difference(dense[0].ptr, dense[1].ptr, out.ptr, 64, h, 64, 64, 64, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    M.bits_equal(out.to_numpy(np.float32, (h, 64)), want[:, :64], "dense")


# ---- the HIP engine's PipelineConfig.ground -------------------------------------------------------------------------------------
WP, HP, NP, RP = 256, 192, 30_000, 3
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU
LOCATIONS = [pcr.MemoryLocation.Host, pcr.MemoryLocation.Device]


def gpu_cfg(location=pcr.MemoryLocation.Host, W=WP, H=HP, **kw):
    cfg = G.pipeline_cfg(W, H, GPU, **kw)
    cfg.result_location = location
    return cfg


def result_bands(pipe):
    res = pipe.result()
    return G.grid_bands(res if res.location() == pcr.MemoryLocation.Host else res.to_host())


def create(cfg, engine="hip"):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == engine
    return pipe


def host_pipeline_bands(clouds, W=WP, H=HP, **kw):
    """The host-engine pipeline's result after each of `clouds` (held to the host loop and the model by the CPU suite)."""
    pipe = create(G.pipeline_cfg(W, H, CPU, **kw), "host")
    out = []
    for c in clouds:
        pipe.ingest(c)
        pipe.finalize()
        out.append(G.grid_bands(pipe.result()))
    return out


@pytest.fixture(scope="module")
def pipe_case():
    c1, c2 = G.cloud(WP, HP, NP, seed=81), G.cloud(WP, HP, NP, seed=82)
    want = {r: host_pipeline_bands([c1, c2], radius=r) for r in (0, RP)}
    raw = host_pipeline_bands([c1, c2], ground=False)
    dtm = want[0][0][3]
    assert np.isnan(raw[0][0]).sum() < np.isnan(dtm).sum() < dtm.size          # the filter removed cells
    return c1, c2, want, raw


@pytest.mark.parametrize("radius", [0, RP])
@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_equals_the_host_engine(pipe_case, location, wait, radius):
    c1, c2, want, raw = pipe_case
    pipe = create(gpu_cfg(location, radius=radius))

    def finalize():
        if wait:
            pipe.finalize()
        else:
            pipe.finalize_async()
            pipe.synchronize()

    pipe.ingest(c1)
    finalize()
    res = pipe.result()
    assert [res.band_desc(b).name for b in range(res.num_bands())] == list(G.BANDS) + ["dtm", "hag"]
    got = result_bands(pipe)
    for b in range(5):
        G.bits_equal(got[b], want[radius][0][b], f"band {b}")
        M.bits_equal(got[b], want[radius][0][b], f"band {b}, NaN bits too")
    # result_band_device() answers for the new bands
    A = load_cabi()
    for b in range(5):
        back = np.empty((HP, WP), np.float32)
        A.check(A.lib().pcr_hip_memcpy_d2h(back.ctypes.data, C.c_void_p(pipe.result_band_device_ptr(b)), back.nbytes, None))
        A.check(A.lib().pcr_hip_stream_synchronize(None))
        M.bits_equal(back, want[radius][0][b], f"result_band_device {b}")
    assert pipe.result_band_device_ptr(5) == 0
    # a second ingest accumulates into raw bands the filter never touched
    pipe.ingest(c2)
    finalize()
    got = result_bands(pipe)
    for b in range(5):
        M.bits_equal(got[b], want[radius][1][b], f"second finalize, band {b}")
    if radius == 0:
        for b in range(3):
            M.bits_equal(got[b], raw[1][b], f"raw band {b} is what a pipeline without ground holds")


@pytest.fixture(scope="module")
def no_top_case(pipe_case):
    c1, c2 = pipe_case[:2]
    return c1, c2, {r: host_pipeline_bands([c1, c2], radius=r, top=False) for r in (0, RP)}


@pytest.mark.parametrize("radius", [0, RP])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_without_a_top_band_equals_the_host_engine(no_top_case, location, radius):
    """A ground plan without a top band: one extra band, the DTM, and no hag band behind it.  Min and Max live in their bands
    as deferred planes after the first ingest, so the second ingest has to find them in the raw bands, not in the filled ones."""
    c1, c2, want = no_top_case
    pipe = create(gpu_cfg(location, radius=radius, top=False))
    A = load_cabi()
    for k, c in enumerate((c1, c2)):
        pipe.ingest(c)
        pipe.finalize()
        res = pipe.result()
        assert [res.band_desc(b).name for b in range(res.num_bands())] == list(G.BANDS) + ["dtm"]
        got = result_bands(pipe)
        assert len(got) == 4
        for b in range(4):
            M.bits_equal(got[b], want[radius][k][b], f"finalize {k + 1}, band {b}")
            back = np.empty((HP, WP), np.float32)
            A.check(A.lib().pcr_hip_memcpy_d2h(back.ctypes.data, C.c_void_p(pipe.result_band_device_ptr(b)), back.nbytes, None))
            A.check(A.lib().pcr_hip_stream_synchronize(None))
            M.bits_equal(back, want[radius][k][b], f"finalize {k + 1}, result_band_device {b}")
        assert pipe.result_band_device_ptr(4) == 0


def test_state_saved_after_a_filtered_finalize_is_the_plain_state(tmp_path, pipe_case):
    c1, _, want, raw = pipe_case
    pipe = create(gpu_cfg())
    pipe.ingest(c1)
    pipe.finalize()
    M.bits_equal(result_bands(pipe)[3], want[0][0][3], "dtm")
    pipe.save_state(str(tmp_path))
    cfg = gpu_cfg(ground=False)
    cfg.state_dir, cfg.resume = str(tmp_path), True
    again = create(cfg)
    again.finalize()
    got = result_bands(again)
    assert len(got) == 3
    for b in range(3):
        M.bits_equal(got[b], raw[0][b], f"resumed without ground, band {b}")


@pytest.mark.parametrize("location", LOCATIONS)
def test_geotiff_and_overview_level_hold_the_new_bands(tmp_path, location):
    Wc, Hc = 520, 512                                                          # write_cog's rule gives a level only from 512 cells a side
    pts = G.cloud(Wc, Hc, 200_000, seed=83)
    want = host_pipeline_bands([pts], W=Wc, H=Hc, radius=2)[0]
    cfg = gpu_cfg(location, W=Wc, H=Hc, radius=2)
    cfg.output_path, cfg.write_cog = str(tmp_path / "g.tif"), True
    pipe = create(cfg)
    pipe.ingest(pts)
    pipe.finalize()
    assert pcr.read_geotiff_overviews(cfg.output_path) == [(260, 256)]
    assert pcr.read_geotiff_band_names(cfg.output_path) == list(G.BANDS) + ["dtm", "hag"]
    got = result_bands(pipe)
    for b in range(5):
        M.bits_equal(got[b], want[b], f"band {b}")
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), want[b], f"file band {b}")
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), M.down(want[b]), f"file band {b} level 1")


def test_out_of_core_equals_in_core(tmp_path, pipe_case):
    c1, _, want, _ = pipe_case
    cfg = gpu_cfg(radius=RP)
    cfg.grid.tile_width = cfg.grid.tile_height = 64
    cfg.grid.compute_dimensions()
    # 2 planes (+ count) + 3 bands of 256 floats per row, 64-row tile rows: 800 KB hold two of the three tile rows
    cfg.gpu_memory_budget = 800_000
    cfg.state_dir = str(tmp_path)
    ooc = create(cfg)
    assert ooc.out_of_core()
    ooc.ingest(c1)
    ooc.finalize()
    got = result_bands(ooc)
    assert len(got) == 5
    for b in range(5):
        M.bits_equal(got[b], want[RP][0][b], f"band {b}")
