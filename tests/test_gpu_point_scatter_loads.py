"""The Point scatter pass (k_bin_scatter) with its value loads in flight together and behind the reservation atomics, the
presence of a value array a property of the instantiation, and the write-out unrolled by four.

None of that changes a result, so every case is a comparison that holds before and after: bands against the oracle to the
tolerances of the other Point tests, `points_valid` exact.  What the cases choose is which code runs: the ends of a chunk
(ragged 4 096-point blocks through the scalar loads, full chunks through the 16-byte loads, sentinel keys inside both), each
of the three launch shapes (asserted through `scatter_chunk` / `num_bins`), no value array at all, a value array that is not
16-byte aligned (every block scalar), and staging rounds that end in a partial group of the unrolled write-out."""
import ctypes as C

import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
from conftest import load_cabi
from test_gpu_finalize_with_scatter import OnHost
from test_gpu_fullgrid_oracle import ALL6, check_point_bands, poison_device_memory
from test_gpu_pipeline_api import cloud_from, config_for, spec

pytestmark = pytest.mark.gpu

W, H = 640, 520                      # as test_gpu_point_step_launches: a few dozen bins, the 512 x 24 shape
CHUNK = 512 * 24                     # 12 288


def run_pipeline(og, x, y, v, names=ALL6):
    poison_device_memory(6 * og.width * og.height * 4)
    p = pcr.Pipeline.create(config_for(og, [spec(t) for t in names], scatter_path=2))
    assert p is not None, pcr.pipeline_create_error()
    p.ingest(cloud_from(x, y, {"value": v}, "device"))
    info = p.last_scatter()
    assert info["path"] == "binned", info
    assert info["points_valid"] == int(np.nansum(O.run(og, O.COUNT, x, y, v)))
    p.finalize()
    check_point_bands(OnHost(p), og, x, y, v, names)
    return info


def cloud(n, w, h, seed, outside=0.1):
    """U(-2, 2) values; `outside` of the points lie beyond the right edge: sentinel keys at random places of every chunk"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, w, n), rng.uniform(0, h, n)
    out = rng.random(n) < outside
    x[out] += w + 5.0
    return x, y, rng.uniform(-2, 2, n).astype(np.float32)


@pytest.mark.parametrize("n", [1, 4095, CHUNK, CHUNK + 1, 3 * CHUNK + 4096 + 37])
def test_chunk_boundaries_of_the_512x24_shape(n):
    og = O.make_grid((0, 0, W, H), tile=(256, 256))
    x, y, v = cloud(n, W, H, 100 + n % 97)
    info = run_pipeline(og, x, y, v)
    assert info["scatter_chunk"] == CHUNK, info


@pytest.mark.parametrize("bins,chunk", [(2100, 1024 * 16), (4100, 1024 * 24)], ids=["1024x16", "1024x24"])
def test_the_two_1024_thread_shapes_on_a_thin_grid(bins, chunk):
    """W = 4 with all four planes: LDS tiles of 128 x 56, one column of them, so H = 56 * bins rows give `bins` bins."""
    w, h = 4, 56 * bins
    og = O.make_grid((0, 0, w, h), tile=(256, 256))
    x, y, v = cloud(2 * chunk + 4096 + 37, w, h, bins)
    info = run_pipeline(og, x, y, v)
    assert info["num_bins"] == bins and tuple(info["lds_tile"]) == (128, 56), info
    assert info["scatter_chunk"] == chunk, info


@pytest.fixture(scope="module")
def A():
    mod = load_cabi()
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def cabi_grid(A, og):
    return A.make_grid((og.min_x, og.min_y, og.max_x, og.max_y), cell=(og.cell_size_x, og.cell_size_y),
                       dims=(og.width, og.height), tile=(og.tile_width, og.tile_height))


def test_no_value_array(A):
    """plane_mask == WGT and d_value NULL: the instantiation that loads no values.  Count exact, through the C ABI (where the
    pointer is ours to pass) and through a Count-only pipeline."""
    n = 3 * CHUNK + 5
    og = O.make_grid((0, 0, W, H), tile=(256, 256))
    x, y, v = cloud(n, W, H, 7)
    want = O.run(og, O.COUNT, x, y, v)
    run = A.ReductionRun(cabi_grid(A, og), A.PLANE_WGT, path=2)
    try:
        dx, dy = A.DeviceBuffer.from_numpy(x), A.DeviceBuffer.from_numpy(y)
        A.check(A.lib().pcr_hip_scatter_point(run.engine, A.PLANE_WGT, C.byref(run.planes), dx.ptr, dy.ptr, None, n))
        A.check(A.lib().pcr_hip_stream_synchronize(None))
        st = run.stats()
        assert st.path == 1 and st.scatter_chunk == CHUNK and st.points_valid == int(np.nansum(want))
        assert np.array_equal(run.finalize(5), want, equal_nan=True)
    finally:
        run.close()
    info = run_pipeline(og, x, y, v, ["Count"])
    assert info["scatter_chunk"] == CHUNK, info


def test_misaligned_value_array_takes_the_scalar_loads_everywhere(A):
    """d_value one float past a 16-byte boundary: no full chunk, every block of 4 096 points loads its values one by one.
    Compared with the aligned run of the same cloud bit for bit, Sum included: the order in which a cell's records are
    added is not defined (the runs of a bin are placed by atomics), so the cloud puts at most one point into a cell."""
    og = O.make_grid((0, 0, W, H), tile=(256, 256))
    n = 3 * CHUNK + 4096 + 37
    rng = np.random.default_rng(21)
    cells = rng.choice(W * H, n, replace=False)                       # one point per cell at the most
    x = (cells % W) + rng.uniform(0.1, 0.9, n)
    y = (cells // W) + rng.uniform(0.1, 0.9, n)
    out = rng.random(n) < 0.1
    x[out] += W + 5.0
    v = rng.uniform(-2, 2, n).astype(np.float32)
    L = A.lib()
    got = {}
    for shift in (0, 1):
        run = A.ReductionRun(cabi_grid(A, og), 15, path=2)
        try:
            dx, dy = A.DeviceBuffer.from_numpy(x), A.DeviceBuffer.from_numpy(y)
            dv = A.DeviceBuffer.from_numpy(np.concatenate([np.zeros(shift, np.float32), v]))
            assert dv.ptr.value % 16 == 0
            A.check(L.pcr_hip_scatter_point(run.engine, 15, C.byref(run.planes), dx.ptr, dy.ptr,
                                            C.c_void_p(dv.ptr.value + 4 * shift), n))
            A.check(L.pcr_hip_stream_synchronize(None))
            st = run.stats()
            assert st.path == 1 and st.scatter_chunk == CHUNK and st.points_valid == int((~out).sum())
            got[shift] = {name: run.finalize(rt) for name, rt in (("Sum", 0), ("Count", 5), ("Max", 1), ("Min", 2))}
        finally:
            run.close()
    for name in ("Sum", "Count", "Max", "Min"):
        assert np.array_equal(got[0][name].view(np.uint32), got[1][name].view(np.uint32)), name
        rt = {"Sum": O.SUM, "Count": O.COUNT, "Max": O.MAX, "Min": O.MIN}[name]
        assert np.array_equal(got[0][name], O.run(og, rt, x, y, v), equal_nan=True), name


def test_window_rounds_that_end_in_a_partial_group():
    """Every valid point in ONE bin, n = 12 288: a full 8 192-record staging round and a partial one of 4 096 records, both
    ending in a single run.  4 096 records are two whole groups of the unrolled write-out for 512 threads, so a second cloud
    of the same size keeps 12 076 points inside: its partial round of 3 884 ends in a group cut short (one whole group, three
    single trips, the last of them with 300 of the 512 threads)."""
    og = O.make_grid((0, 0, W, H), tile=(256, 256))
    rng = np.random.default_rng(33)
    for n, valid in ((CHUNK, CHUNK), (CHUNK, 8192 + 2048 + 3 * 512 + 300)):
        x, y = rng.uniform(130, 250, n), rng.uniform(H - 50, H - 2, n)           # inside one LDS tile (128 columns, >= 52 rows)
        x[valid:] += 2.0 * W
        v = rng.uniform(-2, 2, n).astype(np.float32)
        info = run_pipeline(og, x, y, v)
        assert info["scatter_chunk"] == CHUNK, info
        cnt = O.run(og, O.COUNT, x, y, v)
        tw, th = info["lds_tile"]
        rows, cols = np.nonzero(np.nan_to_num(cnt))
        assert len({(r // th, c // tw) for r, c in zip(rows, cols)}) == 1, "the cloud was meant for one bin"
