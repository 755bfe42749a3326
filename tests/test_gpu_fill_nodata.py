"""fill_nodata on the MI355X: pcr_hip_fill_nodata (hole-free tiles, hole lists, aprons wider than the image and across several
tiles, its scalar variant) behind pcr.fill_nodata on Device grids and through the C-ABI, and the HIP engine's
fill_nodata_radius.  Everything BIT FOR BIT against the host fill, which tests/test_fill_nodata.py holds to the NumPy model of
the contract."""
import ctypes as C

import numpy as np
import pytest

import fill_nodata_common as F
import overviews_common as M
import pcr
from conftest import load_cabi

pytestmark = pytest.mark.gpu

# (cols, rows, bands): the smallest; either side of the 64 x 32 tile; rows that are not 16-byte aligned; three bands
SHAPES = [(1, 1, 1), (3, 5, 1), (63, 65, 1), (64, 64, 1), (65, 129, 1), (257, 130, 1), (301, 203, 3)]
RADII = [1, 7, 32]


def host_and_device(arrays, R, bands=None):
    g = F.make_grid(arrays)
    host = pcr.fill_nodata(g, R, bands)
    dev = pcr.fill_nodata(g.to(pcr.MemoryLocation.Device), R, bands)
    assert dev.location() == pcr.MemoryLocation.Device and host.location() == pcr.MemoryLocation.Host
    return F.grid_bands(host), F.grid_bands(dev.to_host())


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_device_fill_equals_the_host_fill(shape, R):
    w, h, nb = shape
    arrays = [F.values(w, h, seed=w * 100 + h + b + R, nan_fraction=(0.2, 0.9, 0.0)[b % 3]) for b in range(nb)]
    host, dev = host_and_device(arrays, R)
    for b in range(nb):
        F.bits_equal(dev[b], host[b], f"{w}x{h} R={R} band {b}")
    if w * h <= 64 * 64 or R == 1:                                        # (the model is a NumPy loop over the window)
        F.bits_equal(host[0], F.fill(arrays[0], R), "host == model")


@pytest.mark.parametrize("R", [8, 9, 16, 17])                # either side of the kernel's radius classes (LDS sized for 8, 16, 32)
@pytest.mark.parametrize("shape", [(130, 70), (129, 67)])      # 16-byte rows and not
def test_radius_classes(shape, R):
    w, h = shape
    a = F.punch(F.values(w, h, seed=R, nan_fraction=0.3), F.blobs(w, h, 4, 14.0, R), R)
    host, dev = host_and_device([a], R)
    F.bits_equal(dev[0], host[0], f"{w}x{h} R={R}")


def test_device_bands_argument():
    arrays = [F.values(70, 40, seed=s, nan_fraction=0.3) for s in (1, 2, 3)]
    host, dev = host_and_device(arrays, 3, [0, 2])
    for b in range(3):
        F.bits_equal(dev[b], host[b], f"band {b}")
    F.bits_equal(dev[1], arrays[1], "an unlisted band is copied")


# ---- named cases on a 200 x 150 band: tiles are 64 x 32 --------------------------------------------------------------------
W0, H0 = 200, 150


def named_cases():
    base = F.finite_values(W0, H0, seed=5)
    cases = {}
    m = np.zeros((H0, W0), bool)
    m[32:64, 64:128] = True                                               # one tile all NaN between tiles without a NaN
    cases["all-NaN tile next to hole-free tiles"] = F.punch(base, m, 1)
    m = np.zeros((H0, W0), bool)
    m[0, 0] = m[0, W0 - 1] = m[H0 - 1, 0] = m[H0 - 1, W0 - 1] = True
    cases["a hole in each image corner"] = F.punch(base, m, 2)
    m = np.zeros((H0, W0), bool)
    m[:, 63:65] = True                                                    # both sides of a tile border, through every tile row
    m[31:33, :] = True
    cases["hole column and row across every tile border"] = F.punch(base, m, 3)
    cases["95 % NaN"] = F.punch(F.values(W0, H0, seed=6, nan_fraction=0.0), F.isolated(W0, H0, 0.95, 7), 4)
    cases["blobs and full rows"] = F.punch(base, F.blobs(W0, H0, 12, 20.0, 8) | F.full_rows(W0, H0, (0, 77, H0 - 1)), 5)
    return cases


@pytest.fixture(scope="module")
def cases():
    return named_cases()


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("name", list(named_cases()))
def test_named_cases(cases, name, R):
    a = cases[name]
    host, dev = host_and_device([a], R)
    F.bits_equal(dev[0], host[0], f"{name} R={R}")
    keep = ~np.isnan(a)
    F.bits_equal(dev[0][keep], a[keep], "cells that are not NaN are copied")
    if name.startswith("all-NaN tile"):
        # the tile's only valid neighbours are in its apron; deeper than R from its edge nothing is in range
        inner = np.isnan(dev[0])
        want_inner = np.zeros((H0, W0), bool)
        if 32 + R < 64 - R:
            want_inner[32 + R:64 - R, 64 + R:128 - R] = True
        assert (inner == want_inner).all()


# ---- C-ABI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [7, 32])
@pytest.mark.parametrize("offset", [1, 4])                     # an odd float offset: the scalar variant; 4: 16-byte rows, stride 520
def test_cabi_window_in_a_strided_plane_and_guard_words(offset, R):
    A = load_cabi()
    L = A.lib()
    W, H = 200, 136
    stride = 517 if offset == 1 else 520
    plane = F.values(stride, H + 2, seed=91 + offset + R, nan_fraction=0.3)
    src = A.DeviceBuffer.from_numpy(plane)
    window = np.ascontiguousarray(plane.reshape(-1)[offset:offset + H * stride].reshape(H, stride)[:, :W])
    want = F.grid_bands(pcr.fill_nodata(F.make_grid([window]), R))[0]
    sentinel = np.float32(-12345.5)
    out = A.DeviceBuffer.from_numpy(np.full(stride * (H + 2), sentinel, np.float32))
    A.check(L.pcr_hip_fill_nodata(C.c_void_p(src.ptr.value + 4 * offset), C.c_void_p(out.ptr.value + 4 * offset), W, H,
                                  stride, stride, R, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = out.to_numpy()
    inside = np.zeros(stride * (H + 2), bool)
    view = inside[offset:offset + H * stride].reshape(H, stride)
    view[:, :W] = True
    F.bits_equal(got[inside].reshape(H, W), want, "the window")
    assert (got[~inside] == sentinel).all(), "a store outside the window"
    F.bits_equal(src.to_numpy(), plane, "the source is only read")


# ---- the HIP engine's fill_nodata_radius --------------------------------------------------------------------------------------
WP, HP, NP, RP = 256, 192, 4000, 4
GPU = pcr.ExecutionMode.GPU
LOCATIONS = [pcr.MemoryLocation.Host, pcr.MemoryLocation.Device]


def gpu_cfg(radius, location=pcr.MemoryLocation.Host, W=WP, H=HP):
    cfg = F.pipeline_cfg(W, H, GPU, radius)
    cfg.result_location = location
    return cfg


def result_bands(pipe):
    res = pipe.result()
    return F.grid_bands(res if res.location() == pcr.MemoryLocation.Host else res.to_host())


def create(cfg):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "hip"
    return pipe


def host_filled(raw, radius=RP):
    """The host fill (held to the model by the CPU suite) of the Average and Max bands of an unfilled result."""
    g = pcr.fill_nodata(F.make_grid(raw), radius, list(F.FILLED_BANDS))
    return F.grid_bands(g)


@pytest.fixture(scope="module")
def pipe_case():
    c1, c2 = F.cloud(WP, HP, NP, seed=81), F.cloud(WP, HP, NP, seed=82)
    one = create(gpu_cfg(0))
    one.ingest(c1)
    one.finalize()
    raw1 = result_bands(one)
    one.ingest(c2)
    one.finalize()
    raw12 = result_bands(one)
    assert np.isnan(raw1[0]).any() and not np.isnan(raw1[0]).all()
    return c1, c2, raw1, host_filled(raw1), raw12, host_filled(raw12)


@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_result_equals_the_host_fill_of_the_unfilled_result(pipe_case, location, wait):
    c1, _, raw1, want1, _, _ = pipe_case
    pipe = create(gpu_cfg(RP, location))
    pipe.ingest(c1)
    if wait:
        pipe.finalize()
    else:
        pipe.finalize_async()
        pipe.synchronize()
    got = result_bands(pipe)
    for b in range(3):
        F.bits_equal(got[b], want1[b], f"band {b}")
    F.bits_equal(got[1], raw1[1], "Count is untouched")
    assert np.isnan(raw1[0]).sum() > np.isnan(got[0]).sum() > 0
    # result_band_device() is the filled band too
    A = load_cabi()
    for b in range(3):
        back = np.empty((HP, WP), np.float32)
        A.check(A.lib().pcr_hip_memcpy_d2h(back.ctypes.data, C.c_void_p(pipe.result_band_device_ptr(b)), back.nbytes, None))
        A.check(A.lib().pcr_hip_stream_synchronize(None))
        F.bits_equal(back, want1[b], f"result_band_device {b}")


@pytest.mark.parametrize("location", LOCATIONS)
def test_raw_bands_stay_untouched_across_a_second_ingest(pipe_case, location):
    # the first ingest stores the bands with its scatter and leaves planes in them (deferred planes): a fill that wrote the
    # raw bands would come back as accumulation state at the second ingest
    c1, c2, _, want1, raw12, want12 = pipe_case
    pipe = create(gpu_cfg(RP, location))
    pipe.ingest(c1)
    pipe.finalize()
    for b in range(3):
        F.bits_equal(result_bands(pipe)[b], want1[b], f"first finalize, band {b}")
    pipe.ingest(c2)
    pipe.finalize()
    got = result_bands(pipe)
    for b in range(3):
        F.bits_equal(got[b], want12[b], f"second finalize, band {b}")
    F.bits_equal(got[1], raw12[1], "Count is exactly as without fill")
    pipe.finalize()                                                        # and finalize alone changes nothing
    for b in range(3):
        F.bits_equal(result_bands(pipe)[b], want12[b], f"third finalize, band {b}")


def test_state_saved_after_a_filled_finalize_is_the_unfilled_state(tmp_path, pipe_case):
    c1, _, raw1, want1, _, _ = pipe_case
    pipe = create(gpu_cfg(RP))
    pipe.ingest(c1)
    pipe.finalize()
    F.bits_equal(result_bands(pipe)[0], want1[0], "filled")
    pipe.save_state(str(tmp_path))
    cfg = gpu_cfg(0)
    cfg.state_dir, cfg.resume = str(tmp_path), True
    again = create(cfg)
    again.finalize()
    for b in range(3):
        F.bits_equal(result_bands(again)[b], raw1[b], f"resumed without fill, band {b}")


@pytest.mark.parametrize("location", LOCATIONS)
def test_geotiff_and_overview_level_hold_the_filled_bands(tmp_path, location):
    # write_cog's rule gives a level only from 512 cells a side
    Wc, Hc, R = 520, 512, 2
    pts = F.cloud(Wc, Hc, 60_000, seed=83)
    plain = create(gpu_cfg(0, W=Wc, H=Hc))
    plain.ingest(pts)
    plain.finalize()
    want = host_filled(result_bands(plain), R)
    cfg = gpu_cfg(R, location, W=Wc, H=Hc)
    cfg.output_path, cfg.write_cog = str(tmp_path / "f.tif"), True
    pipe = create(cfg)
    pipe.ingest(pts)
    pipe.finalize()
    assert pcr.read_geotiff_overviews(cfg.output_path) == [(260, 256)]
    got = result_bands(pipe)
    for b in range(3):
        F.bits_equal(got[b], want[b], f"band {b}")
        F.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), want[b], f"file band {b}")
        F.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), M.down(want[b]), f"file band {b} level 1")


def test_out_of_core_equals_in_core(tmp_path, pipe_case):
    c1, _, _, want1, _, _ = pipe_case
    cfg = gpu_cfg(RP)
    cfg.grid.tile_width = cfg.grid.tile_height = 64
    cfg.grid.compute_dimensions()
    # 3 planes + 3 bands of 256 floats per row, 64-row tile rows: 800 KB hold two of the three tile rows
    cfg.gpu_memory_budget = 800_000
    cfg.state_dir = str(tmp_path)
    ooc = create(cfg)
    assert ooc.out_of_core()
    ooc.ingest(c1)
    ooc.finalize()
    for b in range(3):
        F.bits_equal(result_bands(ooc)[b], want1[b], f"band {b}")
