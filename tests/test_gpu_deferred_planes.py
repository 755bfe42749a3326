"""State planes the fused Point tile pass leaves in its bands (pcr_hip_engine_defer_planes / pcr_hip_planes_from_bands_if).

A plane whose own reduction (Sum, Count, Max, Min) is an output of its group is a bit-exact function of that band and the
touched flags, so the scatter that defines the planes and stores the bands does not store it; the pipeline puts it back,
once, in front of whatever next reads or changes the state.  What must hold: bands AND planes are, bit for bit, those of the
same calls on a pipeline with finalize_with_first_ingest = False, which never fuses and never defers.

The grid is 512 x 416 cells.  The LDS tiles are 128 columns wide and 96 rows (Sum + Count: 12 bytes per cell) or 128 rows
(Max + Min) tall; the cloud fills columns [0, 150) of rows [0, 300), so with 64 x 64 reference tiles an LDS tile in the second
tile column straddles touched (columns 128..191) and untouched (192..255) reference tiles -- the live-map branch -- the LDS
tiles right of it and below row 320 lie in untouched ones only, and columns 150..191 are empty cells of touched tiles.  16 x 16
reference tiles put more than 64 of them under one LDS tile (the other way into the live map).  Values are multiples of 2^-10
below 1/2: every partial sum is exact in f32 and f64 whatever the order, which is what makes the bitwise comparison fair.
Edge values sit alone in cells of the empty strip: NaN, +Inf with -Inf, -FLT_MAX, +FLT_MAX, -0.0."""
import ctypes as C
import functools

import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
from conftest import load_cabi
from test_gpu_fullgrid_oracle import check_point_bands, poison_device_memory
from test_gpu_pipeline_api import cloud_from, config_for, spec

pytestmark = pytest.mark.gpu

W, H = 512, 416
FLT_MAX = np.float32(3.402823466e+38)
SUM, WGT, MAX, MIN = 1, 2, 4, 8


def at(col, row):
    """world coordinates of the middle of a cell (row 0 is the top row)"""
    return np.asarray(col, dtype=np.float64) + 0.5, H - (np.asarray(row, dtype=np.float64) + 0.5)


def base_cloud(seed, n=250_000, c0=0, r0=0, specials=True):
    rng = np.random.default_rng(seed)
    x = rng.uniform(c0, c0 + 150, n)
    y = H - rng.uniform(r0, r0 + 300, n)
    v = (rng.integers(-511, 512, n) / 1024.0).astype(np.float32)
    if specials:
        cols = np.array([160, 162, 162, 164, 166, 168, 168, 170])
        sx, sy = at(cols + c0, np.full(len(cols), 10 + r0))
        sv = np.array([np.nan, np.inf, -np.inf, -FLT_MAX, FLT_MAX, -0.0, -0.0, 0.25], dtype=np.float32)
        x, y, v = np.concatenate([x, sx]), np.concatenate([y, sy]), np.concatenate([v, sv])
    return x, y, v


def grid(tile=(64, 64), width=W):
    return O.make_grid((0.0, 0.0, float(width), float(H)), tile=tile)


def pipeline(og, names, fused, location="device", **kw):
    cfg = config_for(og, [spec(t) for t in names], scatter_path=2, finalize_with_first_ingest=fused, **kw)
    cfg.result_location = pcr.MemoryLocation.Device if location == "device" else pcr.MemoryLocation.Host
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    return p


def bands_i32(p):
    r = p.result()
    r = r.to_host() if r.location() == pcr.MemoryLocation.Device else r
    return [np.array(r.band_array(b)).view(np.int32) for b in range(r.num_bands())]


def planes_i32(p, width=W):
    """{(group, plane kind): the plane as the pipeline hands it out, int32 view}"""
    A = load_cabi()
    out = {}
    views = p.state_planes()
    for ptr, kind, group in views:
        a = np.empty((p.state_row_count(), width), dtype=np.float32)
        A.check(A.lib().pcr_hip_memcpy_d2h(a.ctypes.data, C.c_void_p(ptr), a.nbytes, None))
        out[(group, kind)] = a
    A.check(A.lib().pcr_hip_device_synchronize())
    return {k: a.view(np.int32) for k, a in out.items()}


def same(got, want, what):
    if isinstance(got, dict):
        assert got.keys() == want.keys(), what
        got, want = [got[k] for k in sorted(got)], [want[k] for k in sorted(want)]
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        bad = g != w
        assert not bad.any(), f"{what} [{i}]: {int(bad.sum())} cells differ, first at {np.argwhere(bad)[0].tolist()}"


def run(p, clouds, sync_between=True):
    """ingest -> finalize for every cloud; sync_between = False: the asynchronous calls, one synchronise at the end"""
    for c in clouds:
        if sync_between:
            p.ingest(c)
            p.finalize()
        else:
            p.ingest_async(c)
            p.finalize_async()
    p.synchronize()


@functools.lru_cache(maxsize=None)
def baseline(names, tile, n_clouds, split=False, width=W):
    """bands and planes of today's plane path (never fused) after n_clouds ingests, each followed by a finalize"""
    p = pipeline(grid(tile, width), names, fused=False)
    run(p, clouds(n_clouds, split))
    got = bands_i32(p), planes_i32(p, width)
    for a in got[0] + list(got[1].values()):
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def clouds(n, split=False):
    first = split_cloud() if split else base_cloud(3)
    second = base_cloud(5, n=200_000, c0=200, r0=100)       # other reference tiles as well: planes AND flags change
    return tuple(cloud_from(x, y, {"value": v}, "device") for x, y, v in (first, second)[:n])


def split_cloud():
    """200 000 points inside columns [10, 110) x rows [100, 190): one LDS tile (rows 96..191 or 0..127) gets more than 2^17
    records, the scan splits its bin, the tile pass merges with atomics and stores no bands"""
    rng = np.random.default_rng(8)
    n = 200_000
    x = np.concatenate([rng.uniform(10, 110, n), rng.uniform(0, 150, 20_000)])
    y = H - np.concatenate([rng.uniform(100, 190, n), rng.uniform(0, 300, 20_000)])
    return x, y, (rng.integers(-511, 512, len(x)) / 1024.0).astype(np.float32)


GROUPS = [(("Sum", "Count", "Average"), SUM | WGT), (("Max", "Min"), MAX | MIN), (("Sum", "Average"), SUM), (("Average",), 0)]


@pytest.mark.parametrize("tile", [(64, 64), (16, 16)], ids=["tile64", "tile16"])
@pytest.mark.parametrize("names,mask", GROUPS, ids=["sum_count_avg", "max_min", "sum_avg", "avg"])
def test_single_ingest_planes_come_back_from_the_bands(names, mask, tile):
    want_bands, want_planes = baseline(names, tile, 1)
    poison_device_memory(6 * W * H * 4)                               # what is not stored must not be read as it lies
    p = pipeline(grid(tile), names, fused=True)
    p.ingest(clouds(1)[0])
    info = p.last_scatter()
    assert info["path"] == "binned" and info["bands_with_scatter"] == 1 and info["deferred_planes"] == mask, info
    p.finalize()
    assert p.last_scatter()["deferred_planes"] == mask                # finalize reads no plane: nothing was put back
    same(bands_i32(p), want_bands, "bands")
    p.finalize()                                                     # again: nothing changes
    same(bands_i32(p), want_bands, "bands, second finalize")
    same(planes_i32(p), want_planes, "planes")
    assert p.last_scatter()["deferred_planes"] == 0 and p.last_scatter()["bands_with_scatter"] == 0
    same(bands_i32(p), want_bands, "bands after the rebuild")


def test_planes_read_before_finalize():
    names = ("Sum", "Count", "Average")
    want_bands, want_planes = baseline(names, (64, 64), 1)
    poison_device_memory(6 * W * H * 4)
    p = pipeline(grid(), names, fused=True)
    p.ingest(clouds(1)[0])
    same(planes_i32(p), want_planes, "planes")
    p.finalize()                                                     # (from the planes: the pointers have left the pipeline)
    same(bands_i32(p), want_bands, "bands")


@pytest.mark.parametrize("sync_between", [True, False], ids=["blocking", "no_host_wait"])
@pytest.mark.parametrize("names,mask", GROUPS[:3], ids=["sum_count_avg", "max_min", "sum_avg"])
def test_a_second_ingest_finds_the_planes(names, mask, sync_between):
    want_bands, want_planes = baseline(names, (64, 64), 2)
    poison_device_memory(6 * W * H * 4)
    p = pipeline(grid(), names, fused=True)
    run(p, clouds(2), sync_between)
    assert p.last_scatter()["deferred_planes"] == 0 and p.last_scatter()["bands_with_scatter"] == 0
    same(bands_i32(p), want_bands, "bands")
    same(planes_i32(p), want_planes, "planes")


@pytest.mark.parametrize("sync_between", [True, False], ids=["blocking", "no_host_wait"])
def test_a_split_bin_stores_the_planes_itself(sync_between):
    names = ("Sum", "Count", "Average")
    want1 = baseline(names, (64, 64), 1, True)
    want2 = baseline(names, (64, 64), 2, True)
    poison_device_memory(6 * W * H * 4)
    p = pipeline(grid(), names, fused=True)
    first, second = clouds(2, True)
    p.ingest(first)
    assert p.last_scatter()["bands_with_scatter"] == 1 and p.last_scatter()["deferred_planes"] == SUM | WGT   # offered and taken ...
    if sync_between:
        p.finalize()
        assert p.last_scatter()["deferred_planes"] == 0               # ... and the device word said the planes were stored
        same(bands_i32(p), want1[0], "bands after the split bin")
    else:
        p.finalize_async()
    run(p, [second], sync_between)                                   # (no host wait: the rebuild is enqueued and returns at once)
    same(bands_i32(p), want2[0], "bands")
    same(planes_i32(p), want2[1], "planes")


def test_host_resident_result():
    names = ("Sum", "Count", "Average")
    want_bands, want_planes = baseline(names, (64, 64), 2)
    poison_device_memory(9 * W * H * 4)
    p = pipeline(grid(), names, fused=True, location="host")
    first, second = clouds(2)
    p.ingest(first)
    assert p.last_scatter()["deferred_planes"] == SUM | WGT
    p.finalize()
    same(bands_i32(p), baseline(names, (64, 64), 1)[0], "bands")
    run(p, [second])
    same(bands_i32(p), want_bands, "bands, second ingest")
    same(planes_i32(p), want_planes, "planes")


@pytest.mark.parametrize("names", [("Sum", "Count", "Average"), ("Max", "Min")], ids=["sum_count_avg", "max_min"])
def test_checkpoint_after_a_single_ingest(names, tmp_path):
    want_bands, want_planes = baseline(names, (64, 64), 1)
    poison_device_memory(6 * W * H * 4)
    p = pipeline(grid(), names, fused=True)
    p.ingest(clouds(1)[0])
    assert p.last_scatter()["deferred_planes"] != 0
    p.save_state(str(tmp_path))
    assert p.last_scatter()["deferred_planes"] == 0
    p.finalize()
    same(bands_i32(p), want_bands, "bands of the pipeline that saved")
    q = pipeline(grid(), names, fused=True)
    q.load_state(str(tmp_path))
    q.finalize()
    same(bands_i32(q), want_bands, "bands of the pipeline that loaded")
    got = planes_i32(q)
    # (a checkpoint holds touched tiles only: elsewhere the loaded planes hold identity values, as the saved ones do)
    same(got, want_planes, "planes of the pipeline that loaded")


def test_a_width_that_is_no_multiple_of_four_defers_nothing():
    names, width = ("Sum", "Count", "Average"), 510
    want_bands, want_planes = baseline(names, (64, 64), 1, False, width)
    p = pipeline(grid(width=width), names, fused=True)
    p.ingest(clouds(1)[0])
    info = p.last_scatter()
    assert info["bands_with_scatter"] == 0 and info["deferred_planes"] == 0, info
    p.finalize()
    same(bands_i32(p), want_bands, "bands")
    same(planes_i32(p, width), want_planes, "planes")


def test_against_the_oracle():
    names = ("Sum", "Count", "Average")
    og = grid()
    x, y, v = base_cloud(3, specials=False)
    x2, y2, v2 = base_cloud(5, n=200_000, c0=200, r0=100, specials=False)
    p = pipeline(og, names, fused=True)
    p.ingest(cloud_from(x, y, {"value": v}, "device"))
    assert p.last_scatter()["deferred_planes"] == SUM | WGT
    p.finalize()
    check_point_bands(type("OnHost", (), {"result": lambda self: p.result().to_host()})(), og, x, y, v, list(names))
    p.ingest(cloud_from(x2, y2, {"value": v2}, "device"))
    p.finalize()
    check_point_bands(type("OnHost", (), {"result": lambda self: p.result().to_host()})(), og, np.concatenate([x, x2]),
                      np.concatenate([y, y2]), np.concatenate([v, v2]), list(names))


def test_cabi_rebuild_honours_the_word_and_a_scatter_without_the_hint_stores_everything():
    A = load_cabi()
    L = A.lib()
    x, y, v = base_cloud(3)
    g = A.make_grid((0.0, 0.0, float(W), float(H)), dims=(W, H), tile=(64, 64))
    cells = W * H

    def scatter(defer):
        run_ = A.ReductionRun(g, 3, path=2)
        outs = [A.DeviceBuffer(cells * 4) for _ in range(3)]
        done = A.DeviceBuffer(4)
        A.check(L.pcr_hip_memset(done.ptr, 0xFF, 4, None))
        for pl in (run_.planes.d_sum, run_.planes.d_wgt):
            A.check(L.pcr_hip_memset(C.c_void_p(pl), 0x7F, cells * 4, None))
        rt = (C.c_int * 3)(A.SUM, A.COUNT, A.AVERAGE)
        po = (C.c_void_p * 3)(*[o.ptr.value for o in outs])
        A.check(L.pcr_hip_engine_planes_fresh(run_.engine, 2))
        A.check(L.pcr_hip_engine_finalize_with_scatter(run_.engine, 3, rt, po, done.ptr))
        if defer is not None:
            A.check(L.pcr_hip_engine_defer_planes(run_.engine, defer))
        run_.scatter(x, y, v)
        return run_, outs, done

    def plane(ptr):
        a = np.empty((H, W), dtype=np.float32)
        A.check(L.pcr_hip_memcpy_d2h(a.ctypes.data, C.c_void_p(ptr), a.nbytes, None))
        A.check(L.pcr_hip_device_synchronize())
        return a.view(np.int32)

    ref, ref_outs, _ = scatter(None)                                  # no hint: today's stores
    try:
        assert L.pcr_hip_engine_finalize_taken(ref.engine) == 1 and L.pcr_hip_engine_planes_deferred(ref.engine) == 0
        want = plane(ref.planes.d_sum), plane(ref.planes.d_wgt)
        assert not (want[0] == 0x7F7F7F7F).any() and not (want[1] == 0x7F7F7F7F).any()
        # MAX is no plane of this scatter and MIN's reduction no band of it: only SUM and WGT are taken
        run_, outs, done = scatter(SUM | WGT | MAX | MIN)
        try:
            assert L.pcr_hip_engine_planes_deferred(run_.engine) == SUM | WGT
            st = A.ScatterStats()
            A.check(L.pcr_hip_engine_stats(run_.engine, C.byref(st)))
            assert st.deferred_planes == SUM | WGT
            assert done.to_numpy(np.uint32, (1,))[0] == 1
            assert (plane(run_.planes.d_sum) == 0x7F7F7F7F).all() and (plane(run_.planes.d_wgt) == 0x7F7F7F7F).all()   # not stored
            _, tp = run_.touched()
            src = (C.c_void_p * 4)(outs[0].ptr.value, outs[1].ptr.value, None, None)
            A.check(L.pcr_hip_memset(done.ptr, 0, 4, None))           # word 0: "the scatter stored the planes" -- a no-op
            A.check(L.pcr_hip_planes_from_bands_if(C.byref(g), C.byref(run_.planes), SUM | WGT, src, tp, done.ptr, None))
            assert (plane(run_.planes.d_sum) == 0x7F7F7F7F).all() and (plane(run_.planes.d_wgt) == 0x7F7F7F7F).all()
            word = np.array([1], dtype=np.uint32)
            A.check(L.pcr_hip_memcpy_h2d(done.ptr, word.ctypes.data, 4, None))
            A.check(L.pcr_hip_planes_from_bands_if(C.byref(g), C.byref(run_.planes), SUM | WGT, src, tp, done.ptr, None))
            assert np.array_equal(plane(run_.planes.d_sum), want[0]) and np.array_equal(plane(run_.planes.d_wgt), want[1])
            run_.scatter(x, y, v)                                     # the hint covered ONE scatter
            assert L.pcr_hip_engine_planes_deferred(run_.engine) == 0
        finally:
            run_.close()
    finally:
        ref.close()
