"""GeoTIFF overviews on the MI355X: pcr_hip_downsample2 (the fused six-level kernel, its scalar variant, the relaunch beyond
six levels) behind build_overviews on Device grids and through the C-ABI, and the HIP engine's write_cog.  Everything BIT FOR
BIT against the host's levels, which tests/test_overviews.py holds to the NumPy model of the contract."""
import ctypes as C

import numpy as np
import pytest

import overviews_common as M
import pcr
from conftest import load_cabi

pytestmark = pytest.mark.gpu

MODES = ["average", "nearest"]
# (cols, rows, bands): the smallest; either side of the 64-cell tile; 16-byte rows with ragged tiles; rows that are not 16-byte
# aligned, three bands; ten levels: the kernel runs twice, the second time on level 6
SHAPES = [(1, 1, 1), (2, 2, 1), (3, 5, 1), (63, 65, 1), (64, 64, 1), (65, 129, 1), (257, 130, 1), (260, 136, 1), (301, 203, 3),
          (1000, 700, 1)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_device_levels_equal_the_host_levels(shape, mode):
    w, h, nb = shape
    arrays = [M.values(w, h, seed=w * 100 + h + b, nan_fraction=(0.2, 0.9, 0.0)[b % 3]) for b in range(nb)]
    g = M.make_grid(arrays)
    n = M.max_levels(w, h)
    host = pcr.build_overviews(g, n, mode)
    dev = pcr.build_overviews(g.to(pcr.MemoryLocation.Device), n, mode)
    assert len(dev) == len(host) == n
    for k in range(n):
        assert dev[k].location() == pcr.MemoryLocation.Device
        back = dev[k].to_host()
        for b in range(nb):
            assert back.band_desc(b).name == g.band_desc(b).name
            M.bits_equal(M.grid_bands(back)[b], M.grid_bands(host[k])[b], f"{w}x{h} {mode} band {b} level {k + 1}")
    if n:
        M.bits_equal(M.grid_bands(host[0])[0], M.down(arrays[0], mode), "host level 1 == model")


@pytest.mark.parametrize("mode", MODES)
def test_fused_levels_equal_the_single_level(mode):
    a = M.values(130, 70, seed=7)
    d = M.make_grid([a]).to(pcr.MemoryLocation.Device)
    one = pcr.build_overviews(d, 1, mode)
    four = pcr.build_overviews(d, 4, mode)
    M.bits_equal(M.grid_bands(one[0].to_host())[0], M.grid_bands(four[0].to_host())[0], "level 1 of 1 and of 4")
    M.bits_equal(M.grid_bands(one[0].to_host())[0], M.down(a, mode), "level 1 == model")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("offset", [1, 4])                     # an odd float offset: the scalar variant; 4: 16-byte rows, stride 520
def test_cabi_window_in_a_strided_plane_and_guard_words(mode, offset):
    A = load_cabi()
    L = A.lib()
    W, H, levels = 200, 136, 8
    stride = 517 if offset == 1 else 520
    plane = M.values(stride, H + 2, seed=91 + offset)
    src = A.DeviceBuffer.from_numpy(plane)
    window = plane.reshape(-1)[offset:offset + H * stride].reshape(H, stride)[:, :W]
    want = M.pyramid(np.ascontiguousarray(window), levels, "nearest" if mode else "average")
    guard, sentinel = 16, np.float32(-12345.5)
    sizes = [wk.size for wk in want]
    starts = np.cumsum([guard] + [s + guard for s in sizes])[:-1]
    total = int(starts[-1] + sizes[-1] + guard)
    out = A.DeviceBuffer.from_numpy(np.full(total, sentinel, np.float32))
    ptrs = (C.c_void_p * levels)(*[out.ptr.value + 4 * int(s) for s in starts])
    A.check(L.pcr_hip_downsample2(C.c_void_p(src.ptr.value + 4 * offset), W, H, stride, ptrs, levels, mode, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = out.to_numpy()
    keep = np.ones(total, bool)
    for s, wk in zip(starts, want):
        M.bits_equal(got[int(s):int(s) + wk.size].reshape(wk.shape), wk, f"level {wk.shape}")
        keep[int(s):int(s) + wk.size] = False
    assert (got[keep] == sentinel).all(), "a store outside a level's plane"
    M.bits_equal(src.to_numpy(), plane, "the source is only read")


# ---- the HIP engine's write_cog ---------------------------------------------------------------------------------------------
def gpu_cfg(W, H, path, location, rows=None):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = pcr.ExecutionMode.GPU
    cfg.result_location = location
    specs = []
    for t in (pcr.ReductionType.Sum, pcr.ReductionType.Average, pcr.ReductionType.Count):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", t
        specs.append(r)
    cfg.reductions = specs
    cfg.output_path, cfg.write_cog = path, True
    if rows:
        cfg.shard_row_begin, cfg.shard_row_end = rows
    return cfg


@pytest.fixture(scope="module")
def points():
    W, H, n = 1040, 520, 200_000
    rng = np.random.default_rng(61)
    c = pcr.PointCloud.create(n)
    c.set_x_array(rng.uniform(0.0, W * 0.8, n))                # the right fifth stays empty: NaN cells
    c.set_y_array(rng.uniform(0.0, H, n))
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", rng.normal(0.0, 100.0, n).astype(np.float32))
    return W, H, c


@pytest.mark.parametrize("location", [pcr.MemoryLocation.Host, pcr.MemoryLocation.Device])
@pytest.mark.parametrize("rows", [None, (130, 390)])
def test_gpu_pipeline_write_cog(tmp_path, points, location, rows):
    from PIL import Image
    W, H, c = points
    p = str(tmp_path / "cog.tif")
    pipe = pcr.Pipeline.create(gpu_cfg(W, H, p, location, rows))
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "hip"
    pipe.ingest(c)
    pipe.finalize()
    res = pipe.result()
    bands = M.grid_bands(res if location == pcr.MemoryLocation.Host else res.to_host())
    h = H if rows is None else rows[1] - rows[0]
    assert bands[0].shape == (h, W) and np.isnan(bands[1]).any() and not np.isnan(bands[1]).all()
    # the reference's rule on the rows this pipeline owns: 520 / 2 >= 256 > 520 / 4; a 260-row block has no level
    sizes = [(520, 260)] if rows is None else []
    assert pcr.read_geotiff_overviews(p) == sizes
    for b in range(3):
        M.bits_equal(pcr.read_geotiff_band(p, b), bands[b], f"band {b} level 0")
        for k, want in enumerate(M.pyramid(bands[b], len(sizes))):
            M.bits_equal(pcr.read_geotiff_band(p, b, k + 1), want, f"band {b} level {k + 1}")
    with Image.open(p) as im:
        assert im.n_frames == 1 + len(sizes)
        for k in range(im.n_frames):
            im.seek(k)
            im.load()
