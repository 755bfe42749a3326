"""Per-cell extremes on the MI355X: both scatter paths of pcr_hip_scatter_extremes and pcr_hip_extremes_band through the C-ABI,
and PipelineConfig::extremes on the HIP engine, against the NumPy model of tests/extremes_common.py and against the host engine.
Every comparison is np.array_equal on uint32 views: the state is a set of keys, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import extremes_common as E
import las_common as LC
import sample_grid_common as S
from conftest import load_cabi

pytestmark = pytest.mark.gpu

pcr = pytest.importorskip("pcr")

G = E.GRID
N = 20_000
INF = float("inf")
LOWEST, HIGHEST = E.LOWEST, E.HIGHEST
DEVICE = pcr.MemoryLocation.Device

# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
# A 300 x 70 state window: three tile columns, the last ragged; three tile rows at k = 8 (tiles of 32 rows), one clipped tile row at
# k = 2 and 4 (144 and 72 rows); 60 % of the points in one cell, more than one work item holds: the scan splits that bin, the
# shared-item merge runs, and that one cell's chain is under heavy contention.
CG = dict(min_x=0.0, min_y=0.0, max_x=300.0, max_y=70.0, cs=1.0, W=300, H=70)
CN = 200_000


@pytest.fixture(scope="module")
def A():
    return load_cabi()


@pytest.fixture(scope="module")
def cclouds():
    """The cloud, and per side a second one whose values are all more extreme (lower for LOWEST, higher for HIGHEST: every slot of
    a cell it reaches is displaced) with a point mask."""
    first = E.make_points(CN, 21, g=CG)
    E.check_cloud(first, CG)
    second = {}
    for side, shift in ((LOWEST, -8.0), (HIGHEST, 8.0)):
        c = E.make_points(CN, 22, g=CG, shift=shift)
        a, b = c["z"][np.isfinite(c["z"])], first["z"][np.isfinite(first["z"])]
        assert a.max() < b.min() if side == LOWEST else a.min() > b.max()
        c["keep"] = (np.random.default_rng(4).random(CN) < 0.7).astype(np.uint8)
        second[side] = c
    return first, second


@pytest.fixture(scope="module")
def model_planes(cclouds):
    """(k, side) -> (planes after the first scatter, planes after the masked second one): computed once, never changed."""
    first, seconds = cclouds
    cache = {}

    def get(k, side):
        if (k, side) not in cache:
            second = seconds[side]
            one = E.planes(CG, first["x"], first["y"], first["z"], k, side)
            both = {n: np.concatenate([first[n], second[n]]) for n in ("x", "y", "z")}
            keep = np.concatenate([np.ones(CN, bool), second["keep"] != 0])
            two = E.planes(CG, both["x"], both["y"], both["z"], k, side, keep)
            for a in (one, two):
                a.setflags(write=False)
            cache[(k, side)] = (one, two)
        return cache[(k, side)]
    return get


class ExtRun:
    """One set of key planes on the device, driven through the C-ABI alone."""

    def __init__(self, A, k, side, path):
        self.A, self.L, self.k, self.side = A, A.lib(), k, side
        self.grid = A.make_grid((0, 0, CG["W"], CG["H"]), dims=(CG["W"], CG["H"]), tile=(256, 64))
        self.keys = A.DeviceBuffer(k * CG["W"] * CG["H"] * 4)
        A.check(self.L.pcr_hip_memset(self.keys.ptr, 0xFF, self.keys.nbytes, None))
        self.engine = C.c_void_p()
        A.check(self.L.pcr_hip_engine_create(C.byref(self.engine), C.byref(self.grid), 0, None))
        A.check(self.L.pcr_hip_engine_set_path(self.engine, path))

    def scatter(self, c, keep=None):
        A, L = self.A, self.L
        bufs = [A.DeviceBuffer.from_numpy(np.asarray(c[n], t)) for n, t in (("x", np.float64), ("y", np.float64), ("z", np.float32))]
        if keep is not None:
            bufs.append(A.DeviceBuffer.from_numpy(np.asarray(keep, np.uint8)))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, bufs[3].ptr if keep is not None else None))
        A.check(L.pcr_hip_scatter_extremes(self.engine, self.keys.ptr, self.k, self.side, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                                           len(c["x"])))
        A.check(L.pcr_hip_stream_synchronize(None))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, None))
        st = A.ScatterStats()
        A.check(L.pcr_hip_engine_stats(self.engine, C.byref(st)))
        return st

    def planes(self):
        return self.keys.to_numpy(np.uint32, (self.k, CG["H"], CG["W"]))

    def close(self):
        self.L.pcr_hip_engine_destroy(self.engine)
        self.keys.free()


def check_three_scatters(A, clouds, want, k, side, path):
    first, second = clouds[0], clouds[1][side]
    run = ExtRun(A, k, side, path)
    try:
        what = f"path {path}, k {k}, side {side}"
        routed = E.route(CG, first["x"], first["y"])[0]
        st = run.scatter(first)
        assert st.path == (1 if path == A.PATH_BINNED else 0), "the path that was asked for did not run"
        assert st.points_in == CN and st.points_valid == int(routed.sum())
        E.keys_equal(run.planes(), want[0], f"{what}: no mask")
        assert (want[0][:, CG["H"] // 2, CG["W"] // 3] != E.EMPTY).all()  # the contended cell (make_points) kept k distinct keys
        st = run.scatter(second, second["keep"])                          # lower values under a point mask: slots are displaced
        routed2 = E.route(CG, second["x"], second["y"])[0]
        assert st.path == (1 if path == A.PATH_BINNED else 0) and st.points_valid == int((routed2 & (second["keep"] != 0)).sum())
        E.keys_equal(run.planes(), want[1], f"{what}: + lower values, masked")
        assert (want[1][0] != want[0][0]).mean() > 0.5
        run.scatter(first)                                                # pure duplicates (or values that cannot enter): nothing changes
        run.scatter(second, second["keep"])
        E.keys_equal(run.planes(), want[1], f"{what}: + duplicates")
        if path == A.PATH_BINNED:
            assert st.lds_tile_w == 128 and st.lds_tile_h == {2: 144, 4: 72, 8: 32}[k] and st.num_bins >= (9 if k == 8 else 3)
    finally:
        run.close()


@pytest.mark.parametrize("side", [LOWEST, HIGHEST], ids=["lowest", "highest"])
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("path", [1, 2], ids=["direct", "binned"])
def test_cabi_both_paths_against_the_model(A, cclouds, model_planes, path, k, side):
    check_three_scatters(A, cclouds, model_planes(k, side), k, side, path)


@pytest.mark.parametrize("mode", ["two_level", "bands"])
def test_cabi_large_grid_forms_on_the_small_grid(A, cclouds, model_planes, monkeypatch, mode):
    monkeypatch.setenv("PCR_HIP_DEBUG_MAX_BINS", "6")                    # read by pcr_hip_engine_create: fewer bins than the 9 tiles
    monkeypatch.setenv("PCR_HIP_DEBUG_TWO_LEVEL", "1" if mode == "two_level" else "0")
    check_three_scatters(A, cclouds, model_planes(8, LOWEST), 8, LOWEST, 2)


@pytest.mark.parametrize("side", [LOWEST, HIGHEST], ids=["lowest", "highest"])
@pytest.mark.parametrize("k", [2, 8])
def test_cabi_band_equals_the_host_twin(A, model_planes, k, side):
    L = A.lib()
    keys = np.ascontiguousarray(model_planes(k, side)[0])
    g = A.make_grid((0, 0, CG["W"], CG["H"]), dims=(CG["W"], CG["H"]), tile=(256, 64))
    cells = CG["W"] * CG["H"]
    d_keys = A.DeviceBuffer.from_numpy(keys)
    for gap in (0.0, 0.5, INF):
        d_out, d_vals = A.DeviceBuffer(cells * 4), A.DeviceBuffer(k * cells * 4)
        h_out, h_vals = np.full((CG["H"], CG["W"]), -1.0, np.float32), np.full((k, CG["H"], CG["W"]), -1.0, np.float32)
        A.check(L.pcr_hip_extremes_band(C.byref(g), d_keys.ptr, k, side, C.c_float(gap), d_out.ptr, d_vals.ptr, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        A.check(L.pcr_hip_extremes_band_host(C.byref(g), keys.ctypes.data, k, side, C.c_float(gap), h_out.ctypes.data, h_vals.ctypes.data))
        got = d_out.to_numpy(np.float32, (CG["H"], CG["W"]))
        E.bits_equal(got, h_out, f"kernel against its host twin, max_gap {gap}")
        E.bits_equal(got, E.band(keys, side, gap), f"kernel against the model, max_gap {gap}")
        E.bits_equal(d_vals.to_numpy(np.float32, (k, CG["H"], CG["W"])), h_vals, "decoded values against the twin")
        E.bits_equal(h_vals, E.value_of(keys, side), "decoded values against the model")
        d_out.free()
        d_vals.free()
    # without the decoded planes
    d_out = A.DeviceBuffer(cells * 4)
    A.check(L.pcr_hip_extremes_band(C.byref(g), d_keys.ptr, k, side, C.c_float(1.0), d_out.ptr, None, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    E.bits_equal(d_out.to_numpy(np.float32, (CG["H"], CG["W"])), E.band(keys, side, 1.0), "band alone")
    assert np.isnan(h_out).any() and (~np.isnan(h_out)).any()
    d_out.free()
    d_keys.free()


# ---- the pipeline on the HIP engine --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points():
    c = E.make_points(N, 11)
    E.check_cloud(c, G)
    return c


def create(cfg, engine="hip"):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == engine
    return p


def run(cfg, clouds, location=None, engine="hip"):
    p = create(cfg, engine)
    for c in clouds:
        p.ingest(E.make_cloud(pcr, c, location))
    return p


def entries():
    return [E.entry(pcr, "z", LOWEST, 4, 1.0), E.entry(pcr, "z", HIGHEST, 8, 0.25), E.entry(pcr, "z", LOWEST, 2, INF, name="z_min")]


SPECS = [(LOWEST, 4, 1.0), (HIGHEST, 8, 0.25), (LOWEST, 2, INF)]


def check_against_model(p, c, keep=None, what=""):
    names, bands = E.result_bands(p)
    assert names == ["z_1", "z_2", "z_low", "z_high", "z_min"]
    for i, (side, k, gap) in enumerate(SPECS):
        want = E.planes(G, c["x"], c["y"], c["z"], k, side, keep)
        E.bits_equal(p.extremes(i), E.value_of(want, side), f"{what}: values of entry {i}")
        E.bits_equal(bands[2 + i], E.band(want, side, gap), f"{what}: band {names[2 + i]}")
    m = ~np.isnan(bands[1])
    assert np.array_equal(E.fold_zero(bands[1])[m], E.bits(bands[4])[m])          # max_gap = +Inf: the Min band (a zero's sign folded)


@pytest.mark.parametrize("location", [None, DEVICE], ids=["host-cloud", "device-cloud"])
@pytest.mark.parametrize("path", [0, 1], ids=["auto", "direct"])
def test_pipeline_values_and_bands_match_the_model(points, path, location):
    p = run(E.make_config(pcr, "gpu", entries(), scatter_path=path), [points], location)
    assert p.last_scatter()["path"] == ("direct" if path == 1 else "binned")
    E.bits_equal(p.extremes(0), E.value_of(E.planes(G, points["x"], points["y"], points["z"], 4, LOWEST), LOWEST), "before any finalize")
    p.finalize()
    check_against_model(p, points, what=f"path {path}")


def test_pipeline_equals_the_host_engine_whatever_the_split(points):
    c = points
    own, cfg_filt = [("ret", "LessEqual", 2.0)], [("cls", "NotEqual", 5.0)]
    ext = lambda: entries() + [E.entry(pcr, "z", HIGHEST, 3, 0.5, name="first_returns_high", filt=own)]
    cpu = run(E.make_config(pcr, "cpu", ext(), cfg_filt=cfg_filt), [c], engine="host")
    whole = run(E.make_config(pcr, "gpu", ext(), cfg_filt=cfg_filt, result_location=DEVICE), [c], DEVICE)
    split = run(E.make_config(pcr, "gpu", ext(), cfg_filt=cfg_filt), [E.take(c, i) for i in E.uneven_splits(N, 7, 5)] +
                [E.take(c, np.arange(0))])
    back = run(E.make_config(pcr, "gpu", ext(), cfg_filt=cfg_filt), [E.take(c, np.arange(N)[::-1])])
    for p in (cpu, whole, split, back):
        p.finalize()
    assert whole.result().location() == DEVICE
    keep = E.keep_mask(c, cfg_filt)
    E.bits_equal(cpu.extremes(0), E.value_of(E.planes(G, c["x"], c["y"], c["z"], 4, LOWEST, keep), LOWEST), "host engine against the model")
    E.bits_equal(cpu.extremes(3), E.value_of(E.planes(G, c["x"], c["y"], c["z"], 3, HIGHEST, keep & E.keep_mask(c, own)), HIGHEST),
                 "filtered entry")
    names, ref = E.result_bands(cpu)
    assert names[2:] == ["z_low", "z_high", "z_min", "first_returns_high"]
    for p, what in ((whole, "device cloud, device result"), (split, "7 ingests"), (back, "reversed")):
        for i in range(4):
            E.bits_equal(p.extremes(i), cpu.extremes(i), f"{what}: values {i} against the host engine")
        for b, (u, w) in enumerate(zip(E.result_bands(p)[1][2:], ref[2:])):
            E.bits_equal(u, w, f"{what}: band {names[2 + b]} against the host engine")


def test_pipeline_filters_and_a_surface_channel(points):
    c = dict(points)
    surf = S.Surface(np.random.default_rng(2).integers(-3, 4, (20, 70)).astype(np.float32), G["min_x"] + 1.0, G["max_y"] - 1.0, 0.9, -0.8)
    surf.band[3, 5] = np.nan
    cfg_filt, own = [("cls", "NotEqual", 5.0)], [("ret", "LessEqual", 2.0), ("hag", "Greater", -2.5)]
    cfg = E.make_config(pcr, "gpu", [E.entry(pcr, "hag", HIGHEST, 4, 0.5, filt=own)], cfg_filt=cfg_filt,
                        surface_channels=[pcr.SurfaceChannelConfig("hag", "z", pcr.SampleMode.Bilinear)])
    p = create(cfg)
    p.set_surface("hag", S.pcr_grid(pcr, surf))
    p.ingest(E.make_cloud(pcr, c, DEVICE))
    p.finalize()
    c["hag"] = S.model(surf, c["x"], c["y"], c["z"], S.BILINEAR)          # the model's own sampled channel
    want = E.planes(G, c["x"], c["y"], c["hag"], 4, HIGHEST, E.keep_mask(c, cfg_filt) & E.keep_mask(c, own))
    E.bits_equal(p.extremes(0), E.value_of(want, HIGHEST), "filters + hag: values")
    names, bands = E.result_bands(p)
    assert names[2] == "hag_high"
    E.bits_equal(bands[2], E.band(want, HIGHEST, 0.5), "filters + hag: band")


def test_pipeline_band_placement_fill_ground_and_terrain(points):
    import histogram_common as H
    c = E.take(points, np.arange(0, N, 7))
    c["z"] = np.where(np.isinf(c["z"]), np.float32(0.5), c["z"])

    def cfg(mode, **kw):
        ground = pcr.GroundFilterConfig()
        ground.source_band, ground.top_band, ground.max_radius_cells = "z_low", "z_high", 2
        t = pcr.TerrainBandConfig()
        t.source_band, t.product = "z_low", pcr.TerrainProduct.Roughness
        out = E.make_config(pcr, mode, [E.entry(pcr, "z", LOWEST, 4, 1.0), E.entry(pcr, "z", HIGHEST, 2, 0.0)], fill_nodata_radius=2,
                            ground=ground, terrain=[t], **kw)
        out.histograms = [H.histogram(pcr, bins=8, qs=[0.5], names=["median"])]
        return out
    cpu = run(cfg("cpu"), [c], engine="host")
    gpu = run(cfg("gpu"), [c])
    dev = run(cfg("gpu", result_location=DEVICE), [c], DEVICE)
    for p in (cpu, gpu, dev):
        p.finalize()
    names, ref = E.result_bands(cpu)
    assert names == ["z_1", "z_2", "median", "z_low", "z_high", "dtm", "hag", "z_low_roughness"]
    raw = [E.band(E.planes(G, c["x"], c["y"], c["z"], 4, LOWEST), LOWEST, 1.0), E.band(E.planes(G, c["x"], c["y"], c["z"], 2, HIGHEST), HIGHEST, 0.0)]
    for p, what in ((gpu, "host result"), (dev, "device result")):
        got_names, got = E.result_bands(p)
        assert got_names == names
        for b in range(len(names)):
            if b < 2:                                                    # (the engines' Max / Min may keep different zeros of a cell)
                assert np.array_equal(E.fold_zero(got[b]), E.fold_zero(ref[b])), f"{what}: band {names[b]} against the host engine"
                continue
            E.bits_equal(got[b], ref[b], f"{what}: band {names[b]} against the host engine")
        for j in range(2):                                               # filled like a Min / Max band: the raw cells stay
            m = ~np.isnan(raw[j])
            assert np.array_equal(E.bits(got[3 + j])[m], E.bits(raw[j])[m]) and np.isnan(got[3 + j]).sum() < np.isnan(raw[j]).sum()


def test_pipeline_finalize_twice_with_an_ingest_in_between(points):
    a, b = E.take(points, np.arange(0, N // 2)), E.take(points, np.arange(N // 2, N))
    b = dict(b, z=(b["z"] - np.float32(1.25)).astype(np.float32))
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    p = run(E.make_config(pcr, "gpu", entries()), [a], DEVICE)
    p.finalize()
    check_against_model(p, a, what="first finalize")
    p.ingest(E.make_cloud(pcr, b))
    p.finalize()
    check_against_model(p, both, what="second finalize")


def test_pipeline_pits_and_birds_on_a_tilted_plane():
    def make(cfg, c):
        p = run(cfg, [c], DEVICE)
        p.finalize()
        return p
    E.check_scene(pcr, make, "gpu")


def test_pipeline_ingest_file_decodes_a_channel_only_the_extremes_name(tmp_path):
    fmt, n = 1, 6000
    rng = np.random.default_rng(9)
    f = LC.make_fields(fmt, n, rng)
    f["X"] = rng.integers(-500, 17_000, n).astype(np.int32)
    f["Y"] = rng.integers(-500, 10_000, n).astype(np.int32)
    f["Z"] = rng.integers(-100, 300, n).astype(np.int32)
    scale, offset = (0.001, 0.001, 0.125), (G["min_x"], G["min_y"], 0.0)
    path = str(tmp_path / "tile.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset)
    want = LC.expected(fmt, f, scale, offset, 0.0)
    cfg = E.make_config(pcr, "gpu", [E.entry(pcr, "z", LOWEST, 4, 1.0)], reductions=(("intensity", "Count"), ("intensity", "Max")))
    p = create(cfg)
    assert p.ingest_file(path, 2500) == n
    p.finalize()
    keys = E.planes(G, want["x"], want["y"], want["z"], 4, LOWEST)
    E.bits_equal(p.extremes(0), E.value_of(keys, LOWEST), "ingest_file: values")
    names, bands = E.result_bands(p)
    assert names[2] == "z_low"
    E.bits_equal(bands[2], E.band(keys, LOWEST, 1.0), "ingest_file: band")
    assert (keys[3] != E.EMPTY).mean() > 0.5


def test_a_budget_too_small_for_the_planes_refuses(points):
    small = 12 * G["W"] * G["H"] * 4                                     # room for the planes and bands, not for 8 key planes more
    ok = E.make_config(pcr, "gpu", [], gpu_memory_budget=small)
    assert not create(ok).out_of_core()
    cfg = E.make_config(pcr, "gpu", [E.entry(pcr, k=8)], gpu_memory_budget=small)
    assert pcr.Pipeline.create(cfg) is None
    assert "extremes are not supported on a pipeline that runs out of core" in pcr.pipeline_create_error()
    cfg.gpu_memory_budget = 0
    assert not create(cfg).out_of_core()


def test_checkpoints_are_refused_on_the_hip_engine(points, tmp_path):
    p = run(E.make_config(pcr, "gpu", [E.entry(pcr)]), [points])
    for call in (p.save_state, p.load_state):
        with pytest.raises(RuntimeError, match="checkpoints do not carry the extremes"):
            call(str(tmp_path))


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_auto_path_against_the_host_engine():
    W = 4096
    g = dict(min_x=0.0, min_y=0.0, max_x=float(W), max_y=float(W), cs=1.0, W=W, H=W, tw=4096, th=4096)
    n, k = 10_000_000, 4
    rng = np.random.default_rng(33)
    x, y = rng.uniform(-8.0, W + 8.0, n), rng.uniform(-8.0, W + 8.0, n)
    z = (np.round(rng.standard_normal(n) * 48.0) * 0.25 + 30.0).astype(np.float32)
    z[rng.integers(0, n, 1000)] = np.nan
    cloud = dict(x=x, y=y, z=z)
    cfg = lambda mode, **kw: E.make_config(pcr, mode, [E.entry(pcr, "z", LOWEST, k, 1.0)], g=g, reductions=(("z", "Count"),), **kw)
    gpu = run(cfg("gpu", result_location=DEVICE), [cloud], DEVICE)
    assert gpu.last_scatter()["path"] == "binned"
    cpu = run(cfg("cpu"), [cloud], engine="host")
    gpu.finalize()
    cpu.finalize()
    got = gpu.extremes(0)
    assert got.shape == (k, W, W)
    E.bits_equal(got, cpu.extremes(0), "values against the host engine")
    E.bits_equal(E.result_bands(gpu)[1][1], E.result_bands(cpu)[1][1], "band against the host engine")
    assert (~np.isnan(got[1])).mean() > 0.05 and np.isnan(got[0]).any()
