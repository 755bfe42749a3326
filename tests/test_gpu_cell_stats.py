"""Per-cell stats on the MI355X: both scatter paths of pcr_hip_scatter_cell_stats and pcr_hip_cell_stats_bands through the C-ABI,
and PipelineConfig::cell_stats on the HIP engine, against the model of tests/cell_stats_common.py and against the host engine.
States are compared with np.array_equal on the integer planes, bands on uint32 views: no tolerance anywhere but in the one
scenario at the end, whose bounds are derived in cell_stats_common.check_scene.  (On the preset state "N = 3e9, S1 ~ +-2^52":
tests/test_cell_stats_host.py's docstring.)"""
import ctypes as C

import numpy as np
import pytest

import cell_stats_common as K
from conftest import load_cabi

pytestmark = pytest.mark.gpu

pcr = pytest.importorskip("pcr")

G = K.GRID
MEAN, VARIANCE, STDDEV = K.MEAN, K.VARIANCE, K.STDDEV
DEVICE = pcr.MemoryLocation.Device
ORIGIN, RES = -2.0, 2.0 ** -6

# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
# A 300 x 150 state window under LDS tiles of 128 x 72: three tile columns, the last ragged (128 + 128 + 44), three tile rows, the
# last ragged (72 + 72 + 6); 60 % of 200 000 points in ONE cell: that bin exceeds 2^16 records, the scan splits it, and the
# shared-item merge runs under contention.  Every width is a multiple of 4: the exclusive merge is the 16-byte one.
CG = dict(min_x=0.0, min_y=0.0, max_x=300.0, max_y=150.0, cs=1.0, W=300, H=150)
CN = 200_000
# ... and 301 x 80 with 20 000 points: a width that is no multiple of 4, the one-lane-per-cell merge; nothing is split.
CG2 = dict(min_x=0.0, min_y=0.0, max_x=301.0, max_y=80.0, cs=1.0, W=301, H=80)
CN2 = 20_000
PATHS = pytest.mark.parametrize("path", [1, 2], ids=["direct", "binned"])


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def two_clouds(g, n, seed):
    first = K.make_points(n, seed, g=g)
    K.check_cloud(first, g)
    second = K.make_points(n, seed + 1, g=g)
    second["keep"] = (np.random.default_rng(4).random(n) < 0.7).astype(np.uint8)
    one = K.planes(g, first["x"], first["y"], first["z"], ORIGIN, RES)
    two = K.planes(g, second["x"], second["y"], second["z"], ORIGIN, RES, second["keep"] != 0, into=one)
    for a in one + two:
        a.setflags(write=False)
    return first, second, one, two


@pytest.fixture(scope="module")
def big():
    """(first cloud, masked second cloud, the model after the first, after both): computed once, never changed."""
    return two_clouds(CG, CN, 21)


@pytest.fixture(scope="module")
def odd():
    return two_clouds(CG2, CN2, 31)


class StatRun:
    """One set of the three planes on the device, driven through the C-ABI alone."""

    def __init__(self, A, g, path, preset=None):
        self.A, self.L, self.g = A, A.lib(), g
        self.grid = A.make_grid((0, 0, g["W"], g["H"]), dims=(g["W"], g["H"]), tile=(256, 64))
        shape = (g["H"], g["W"])
        host = preset if preset is not None else (np.zeros(shape, np.uint32), np.zeros(shape, np.int64), np.zeros(shape, np.uint64))
        self.bufs = [A.DeviceBuffer.from_numpy(np.ascontiguousarray(a)) for a in host]
        self.engine = C.c_void_p()
        A.check(self.L.pcr_hip_engine_create(C.byref(self.engine), C.byref(self.grid), 0, None))
        A.check(self.L.pcr_hip_engine_set_path(self.engine, path))

    def scatter(self, c, keep=None):
        A, L = self.A, self.L
        pts = [A.DeviceBuffer.from_numpy(np.asarray(c[n], t)) for n, t in (("x", np.float64), ("y", np.float64), ("z", np.float32))]
        if keep is not None:
            pts.append(A.DeviceBuffer.from_numpy(np.asarray(keep, np.uint8)))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, pts[3].ptr if keep is not None else None))
        A.check(L.pcr_hip_scatter_cell_stats(self.engine, self.bufs[0].ptr, self.bufs[1].ptr, self.bufs[2].ptr, ORIGIN, 1.0 / RES,
                                             pts[0].ptr, pts[1].ptr, pts[2].ptr, len(c["x"])))
        A.check(L.pcr_hip_stream_synchronize(None))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, None))
        st = A.ScatterStats()
        A.check(L.pcr_hip_engine_stats(self.engine, C.byref(st)))
        return st

    def planes(self):
        shape = (self.g["H"], self.g["W"])
        return tuple(b.to_numpy(t, shape) for b, t in zip(self.bufs, (np.uint32, np.int64, np.uint64)))

    def close(self):
        self.L.pcr_hip_engine_destroy(self.engine)
        for b in self.bufs:
            b.free()


def check_two_scatters(A, g, clouds, path, tile_rows):
    first, second, one, two = clouds
    n = len(first["x"])
    run = StatRun(A, g, path)
    try:
        what = f"path {path}, {g['W']} x {g['H']}"
        st = run.scatter(first)
        assert st.path == (1 if path == A.PATH_BINNED else 0), "the path that was asked for did not run"
        assert st.points_in == n and st.points_valid == int(K.route(g, first["x"], first["y"])[0].sum())
        K.planes_equal(run.planes(), one, f"{what}: no mask")
        st = run.scatter(second, second["keep"])
        routed2 = K.route(g, second["x"], second["y"])[0]
        assert st.path == (1 if path == A.PATH_BINNED else 0) and st.points_valid == int((routed2 & (second["keep"] != 0)).sum())
        K.planes_equal(run.planes(), two, f"{what}: + a second cloud, masked")
        assert (two[0] > one[0]).sum() > 1000
        if path == A.PATH_BINNED:
            assert st.lds_tile_w == 128 and st.lds_tile_h == 72 and st.num_bins >= 3 * tile_rows
    finally:
        run.close()


@PATHS
def test_cabi_both_paths_against_the_model(A, big, path):
    hot = big[2][0][CG["H"] // 2, CG["W"] // 3]
    assert hot > 65536, "the contended cell must hold more accepted points than one work item takes"
    check_two_scatters(A, CG, big, path, 3)


@PATHS
def test_cabi_a_width_that_is_no_multiple_of_4(A, odd, path):
    check_two_scatters(A, CG2, odd, path, 2)


@pytest.mark.parametrize("mode", ["two_level", "bands"])
def test_cabi_large_grid_forms_on_the_small_grid(A, big, monkeypatch, mode):
    monkeypatch.setenv("PCR_HIP_DEBUG_MAX_BINS", "6")                    # read by pcr_hip_engine_create: fewer bins than the 9 tiles
    monkeypatch.setenv("PCR_HIP_DEBUG_TWO_LEVEL", "1" if mode == "two_level" else "0")
    check_two_scatters(A, CG, big, 2, 3)


@PATHS
@pytest.mark.parametrize("which", ["big", "odd"])
def test_cabi_carries_across_the_32_bit_boundary(A, big, odd, path, which):
    """Preset planes, one scatter, the sum: S2 = 2^32 - 1, S1 = -1 and N = 2^31 together, then S1 = 2^32 - 1 -- the 64-bit adds
    carry (or borrow) across the 32-bit boundary in the shared merge (the split bin of the large cloud), the 16-byte exclusive
    merge (300 wide) and the one-lane-per-cell merge (301 wide), and in the direct path's atomics."""
    g, clouds = (CG, big) if which == "big" else (CG2, odd)
    first, want = clouds[0], clouds[2]
    shape = (g["H"], g["W"])
    for n0, s10, s20 in ((1 << 31, -1, (1 << 32) - 1), (0, (1 << 32) - 1, 0)):
        preset = (np.full(shape, n0, np.uint32), np.full(shape, s10, np.int64), np.full(shape, s20, np.uint64))
        run = StatRun(A, g, path, preset)
        try:
            run.scatter(first)
            with np.errstate(over="ignore"):
                K.planes_equal(run.planes(), (preset[0] + want[0], preset[1] + want[1], preset[2] + want[2]),
                               f"path {path}, {which}: preset N {n0}, S1 {s10}, S2 {s20}")
            assert ((preset[2] + want[2]) >> np.uint64(32)).any() and (want[1] > 0).any() and (want[1] < 0).any()
        finally:
            run.close()


def device_bands(A, n, s1, s2, origin, res, ddof, products):
    L = A.lib()
    h, w = n.shape
    g = A.make_grid((0, 0, w, h), dims=(w, h), tile=(w, h))
    d = [A.DeviceBuffer.from_numpy(np.ascontiguousarray(a)) for a in (n, s1, s2)]
    outs = [A.DeviceBuffer(h * w * 4) for _ in products]
    for o in outs:
        A.check(L.pcr_hip_memset(o.ptr, 0x55, o.nbytes, None))
    prods = (C.c_int * len(products))(*products)
    ptrs = (C.c_void_p * len(products))(*[o.ptr.value for o in outs])
    A.check(L.pcr_hip_cell_stats_bands(C.byref(g), d[0].ptr, d[1].ptr, d[2].ptr, origin, res, ddof, len(products), prods, ptrs, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = [o.to_numpy(np.float32, (h, w)) for o in outs]
    for b in d + outs:
        b.free()
    return got


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("origin,res", [(0.0, 0.01), (-2.0, 2.0 ** -6), (1500.0, 0.001)])
def test_cabi_bands_equal_the_host_twin_and_the_model(A, origin, res, ddof):
    n, s1, s2 = K.preset_states()
    model = K.bands(n, s1, s2, origin, res, ddof)
    for products in ([MEAN, VARIANCE, STDDEV], [STDDEV, VARIANCE, MEAN], [VARIANCE]):
        got = device_bands(A, n, s1, s2, origin, res, ddof, products)
        twin = K.twin_bands(A, n, s1, s2, origin, res, ddof, products)
        for u, t, k in zip(got, twin, products):
            K.bits_equal(u, t, f"kernel against its host twin: product {k} of {products}, ddof {ddof}")
            K.bits_equal(u, model[k], f"kernel against the model: product {k} of {products}, ddof {ddof}")


def test_cabi_bands_of_a_scattered_state(A, big):
    n, s1, s2 = big[3]
    for ddof in (0, 1):
        got = device_bands(A, n, s1, s2, ORIGIN, RES, ddof, [MEAN, VARIANCE, STDDEV])
        twin = K.twin_bands(A, n, s1, s2, ORIGIN, RES, ddof, [MEAN, VARIANCE, STDDEV])
        model = K.bands(n, s1, s2, ORIGIN, RES, ddof)
        for u, t, k in zip(got, twin, (MEAN, VARIANCE, STDDEV)):
            K.bits_equal(u, t, f"kernel against its host twin, ddof {ddof}")
            K.bits_equal(u, model[k], f"kernel against the model, ddof {ddof}")
        assert np.isnan(got[2]).any() and (~np.isnan(got[2])).any()


# ---- the pipeline on the HIP engine --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points():
    return K.pipeline_points()


def run(cfg, clouds, location=None, engine="hip"):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == engine
    for c in clouds:
        p.ingest(K.make_cloud(pcr, c, location))
    return p


@pytest.mark.parametrize("location", [None, DEVICE], ids=["host-cloud", "device-cloud"])
@pytest.mark.parametrize("path", [0, 1], ids=["auto", "direct"])
def test_pipeline_states_and_bands_match_the_model(points, path, location):
    p = run(K.make_config(pcr, "gpu", K.entries(pcr), scatter_path=path), [points], location)
    assert p.last_scatter()["path"] == ("direct" if path == 1 else "binned")
    origin, res = K.SPECS[0][:2]
    K.planes_equal(p.cell_stats(0), K.planes(G, points["x"], points["y"], points["z"], origin, res), "before any finalize")
    p.finalize()
    K.check_against_model(p, points, what=f"path {path}")


def test_pipeline_model_splits_order_and_a_filtered_entry(points):
    K.scenario_model_and_splits(pcr, "gpu", run, points)


def test_pipeline_equals_the_host_engine(points):
    cfg_filt = [("cls", "NotEqual", 5.0)]
    cpu = run(K.make_config(pcr, "cpu", K.entries(pcr), cfg_filt=cfg_filt), [points], engine="host")
    gpu = run(K.make_config(pcr, "gpu", K.entries(pcr), cfg_filt=cfg_filt, result_location=DEVICE), [points], DEVICE)
    cpu.finalize()
    gpu.finalize()
    assert gpu.result().location() == DEVICE
    names, ref = K.result_bands(cpu)
    for i in range(len(K.SPECS)):
        K.planes_equal(gpu.cell_stats(i), cpu.cell_stats(i), f"state {i} against the host engine")
    for b, (u, w) in enumerate(zip(K.result_bands(gpu)[1][2:], ref[2:])):
        K.bits_equal(u, w, f"band {names[2 + b]} against the host engine")


def test_pipeline_a_surface_channel_as_value_channel(points):
    K.scenario_surface_channel(pcr, "gpu", run, points)


def test_pipeline_band_order_fill_and_terrain_on_the_mean(points):
    names, got = K.scenario_band_order_fill_and_terrain(pcr, "gpu", run, points)
    _, ref = K.scenario_band_order_fill_and_terrain(pcr, "cpu", lambda cfg, clouds: run(cfg, clouds, engine="host"), points)
    for b in range(2, len(names)):                                       # (the engines' Max / Min may keep different zeros of a cell)
        K.bits_equal(got[b], ref[b], f"band {names[b]} against the host engine")


def test_pipeline_ingest_file_decodes_a_channel_only_the_entry_names(tmp_path):
    K.scenario_ingest_file(pcr, "gpu", run, tmp_path)


def test_pipeline_finalize_twice_with_an_ingest_in_between(points):
    n = len(points["x"])
    a, b = K.take(points, np.arange(0, n // 2)), K.take(points, np.arange(n // 2, n))
    p = run(K.make_config(pcr, "gpu", K.entries(pcr)), [a], DEVICE)
    p.finalize()
    K.check_against_model(p, a, what="first finalize")
    p.ingest(K.make_cloud(pcr, b))
    p.finalize()
    K.check_against_model(p, points, what="second finalize")


def test_create_refuses_by_message_on_the_hip_engine():
    K.scenario_refusals(pcr, "gpu")


def test_a_budget_too_small_for_the_planes_refuses():
    small = 12 * G["W"] * G["H"] * 4                                     # room for the planes and bands, not for 4 x 20 bytes a cell more
    ok = K.make_config(pcr, "gpu", [], gpu_memory_budget=small)
    p = pcr.Pipeline.create(ok)
    assert p is not None and not p.out_of_core()
    cfg = K.make_config(pcr, "gpu", [K.entry(pcr, names=[f"s{j}"]) for j in range(4)], gpu_memory_budget=small)
    assert pcr.Pipeline.create(cfg) is None
    assert "cell_stats are not supported on a pipeline that runs out of core" in pcr.pipeline_create_error()
    cfg.gpu_memory_budget = 0
    p = pcr.Pipeline.create(cfg)
    assert p is not None and not p.out_of_core()


def test_checkpoints_are_refused_on_the_hip_engine(points, tmp_path):
    K.scenario_checkpoints_refused(pcr, "gpu", run, points, tmp_path)


# ---- the scenario that shows the point ----------------------------------------------------------------------------------------
def test_pipeline_a_decimetre_of_noise_at_1500_metres():
    def make(cfg, c):
        p = run(cfg, [c], DEVICE)
        p.finalize()
        return p
    K.check_scene(pcr, make, "gpu")
