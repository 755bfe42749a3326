"""Per-cell histograms on the MI355X: both scatter paths of pcr_hip_scatter_histogram and pcr_hip_histogram_percentiles through
the C-ABI, and PipelineConfig::histograms on the HIP engine, against the NumPy model of tests/histogram_common.py and against
the host engine.  Every comparison is np.array_equal on uint32 views: the fold is integer addition, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import histogram_common as H
import las_common as LC
import sample_grid_common as S
from conftest import load_cabi

pytestmark = pytest.mark.gpu

pcr = pytest.importorskip("pcr")

G, QS, LO, HI = H.GRID, H.PERCENTILES, H.LO, H.HI
N = 20_000
DEVICE = pcr.MemoryLocation.Device

# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
# A 300 x 70 state window: three tile columns, the last ragged, and several tile rows at every tile height; 60 % of the points in
# one cell, more than one work item holds: the scan splits that bin and the shared-item merge runs.
CG = dict(min_x=0.0, min_y=0.0, max_x=300.0, max_y=70.0, cs=1.0, W=300, H=70)
CN = 200_000


@pytest.fixture(scope="module")
def A():
    return load_cabi()


@pytest.fixture(scope="module")
def cpoints():
    c = H.make_points(CN, 21, g=CG)
    c["keep"] = (np.random.default_rng(4).random(CN) < 0.7).astype(np.uint8)
    return c


@pytest.fixture(scope="module")
def model_cubes(cpoints):
    """bins -> (cube of the whole cloud, cube of the masked cloud): computed once, never changed."""
    c = cpoints
    out = {}
    for bins in (1, 37, 256):
        out[bins] = (H.cube(CG, c["x"], c["y"], c["z"], LO, HI, bins), H.cube(CG, c["x"], c["y"], c["z"], LO, HI, bins, c["keep"] != 0))
        for a in out[bins]:
            a.setflags(write=False)
    return out


class HistRun:
    """One cube on the device, driven through the C-ABI alone."""

    def __init__(self, A, bins, path):
        self.A, self.L, self.bins = A, A.lib(), bins
        self.grid = A.make_grid((0, 0, CG["W"], CG["H"]), dims=(CG["W"], CG["H"]), tile=(256, 64))
        self.cube = A.DeviceBuffer(bins * CG["W"] * CG["H"] * 4)
        A.check(self.L.pcr_hip_memset(self.cube.ptr, 0, self.cube.nbytes, None))
        self.engine = C.c_void_p()
        A.check(self.L.pcr_hip_engine_create(C.byref(self.engine), C.byref(self.grid), 0, None))
        A.check(self.L.pcr_hip_engine_set_path(self.engine, path))
        self.inv_w = float(np.float64(bins) / (np.float64(np.float32(HI)) - np.float64(np.float32(LO))))

    def scatter(self, c, keep=None):
        A, L = self.A, self.L
        bufs = [A.DeviceBuffer.from_numpy(np.asarray(c[k], t)) for k, t in (("x", np.float64), ("y", np.float64), ("z", np.float32))]
        if keep is not None:
            bufs.append(A.DeviceBuffer.from_numpy(np.asarray(keep, np.uint8)))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, bufs[3].ptr if keep is not None else None))
        A.check(L.pcr_hip_scatter_histogram(self.engine, self.cube.ptr, self.bins, float(np.float32(LO)), self.inv_w, bufs[0].ptr,
                                            bufs[1].ptr, bufs[2].ptr, len(c["x"])))
        A.check(L.pcr_hip_stream_synchronize(None))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, None))
        st = A.ScatterStats()
        A.check(L.pcr_hip_engine_stats(self.engine, C.byref(st)))
        return st

    def counts(self):
        return self.cube.to_numpy(np.uint32, (self.bins, CG["H"], CG["W"]))

    def close(self):
        self.L.pcr_hip_engine_destroy(self.engine)
        self.cube.free()


def check_two_scatters(A, c, cubes, bins, path):
    run = HistRun(A, bins, path)
    try:
        routed = H.route(CG, c["x"], c["y"])[0]
        st = run.scatter(c)
        assert st.path == (1 if path == A.PATH_BINNED else 0), "the path that was asked for did not run"
        assert st.points_in == CN and st.points_valid == int(routed.sum())
        H.cubes_equal(run.counts(), cubes[0], f"path {path}, bins {bins}: no mask")
        st = run.scatter(c, c["keep"])                                   # a second scatter into the same cube, under a point mask
        assert st.path == (1 if path == A.PATH_BINNED else 0) and st.points_valid == int((routed & (c["keep"] != 0)).sum())
        H.cubes_equal(run.counts(), cubes[0] + cubes[1], f"path {path}, bins {bins}: + masked")
        if path == A.PATH_BINNED:
            assert st.lds_tile_w == 128 and st.lds_tile_h in (8, 16, 32) and st.num_bins >= 9
    finally:
        run.close()


@pytest.mark.parametrize("bins", [1, 37, 256])
@pytest.mark.parametrize("path", [1, 2], ids=["direct", "binned"])
def test_cabi_both_paths_against_the_model(A, cpoints, model_cubes, path, bins):
    check_two_scatters(A, cpoints, model_cubes[bins], bins, path)


@pytest.mark.parametrize("mode", ["two_level", "bands"])
def test_cabi_large_grid_forms_on_the_small_grid(A, cpoints, model_cubes, monkeypatch, mode):
    monkeypatch.setenv("PCR_HIP_DEBUG_MAX_BINS", "6")                    # read by pcr_hip_engine_create: fewer bins than tiles
    monkeypatch.setenv("PCR_HIP_DEBUG_TWO_LEVEL", "1" if mode == "two_level" else "0")
    check_two_scatters(A, cpoints, model_cubes[37], 37, 2)


@pytest.mark.parametrize("n_q", [5, 16])
def test_cabi_percentiles_equal_the_host_twin(A, model_cubes, n_q):
    L = A.lib()
    bins = 37
    counts = np.ascontiguousarray(model_cubes[bins][0])
    qs = np.asarray(QS if n_q == 5 else [k / 15.0 for k in range(16)], np.float32)
    g = A.make_grid((0, 0, CG["W"], CG["H"]), dims=(CG["W"], CG["H"]), tile=(256, 64))
    w = float((np.float64(np.float32(HI)) - np.float64(np.float32(LO))) / bins)
    d_counts = A.DeviceBuffer.from_numpy(counts)
    d_outs = [A.DeviceBuffer(CG["W"] * CG["H"] * 4) for _ in qs]
    h_outs = [np.full((CG["H"], CG["W"]), -1.0, np.float32) for _ in qs]
    A.check(L.pcr_hip_histogram_percentiles(C.byref(g), d_counts.ptr, bins, float(np.float32(LO)), w, n_q, qs.ctypes.data,
                                            (C.c_void_p * n_q)(*[b.ptr for b in d_outs]), None))
    A.check(L.pcr_hip_stream_synchronize(None))
    A.check(L.pcr_hip_histogram_percentiles_host(C.byref(g), counts.ctypes.data, bins, float(np.float32(LO)), w, n_q, qs.ctypes.data,
                                                 (C.c_void_p * n_q)(*[o.ctypes.data for o in h_outs])))
    want = H.percentiles(counts, LO, HI, bins, qs)
    for j in range(n_q):
        got = d_outs[j].to_numpy(np.float32, (CG["H"], CG["W"]))
        H.bits_equal(got, h_outs[j], f"kernel against its host twin, q {qs[j]}")
        H.bits_equal(got, want[j], f"kernel against the model, q {qs[j]}")
    assert np.isnan(h_outs[0]).any() and (~np.isnan(h_outs[0])).any()


# ---- the pipeline on the HIP engine --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points():
    return H.make_points(N, 11)


def create(cfg, engine="hip"):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == engine
    return p


def run(cfg, clouds, location=None, engine="hip"):
    p = create(cfg, engine)
    for c in clouds:
        p.ingest(H.make_cloud(pcr, c, location))
    return p


def check_against_model(p, c, bins, keep=None, channel="z", what=""):
    want = H.cube(G, c["x"], c["y"], c[channel], LO, HI, bins, keep)
    H.cubes_equal(p.histogram(0), want, what + " cube")
    names, bands = H.result_bands(p)
    for j, wb in enumerate(H.percentiles(want, LO, HI, bins, QS)):
        assert names[2 + j] == H.band_name(channel, QS[j])
        H.bits_equal(bands[2 + j], wb, f"{what} band {names[2 + j]}")


@pytest.mark.parametrize("location", [None, DEVICE], ids=["host-cloud", "device-cloud"])
@pytest.mark.parametrize("path,bins", [(0, 1), (0, 37), (0, 256), (1, 37)])
def test_pipeline_cube_and_bands_match_the_model(points, path, bins, location):
    p = run(H.make_config(pcr, "gpu", [H.histogram(pcr, bins=bins)], scatter_path=path), [points], location)
    assert p.last_scatter()["path"] == ("direct" if path == 1 else "binned")
    H.cubes_equal(p.histogram(0), H.cube(G, points["x"], points["y"], points["z"], LO, HI, bins), "before any finalize")
    p.finalize()
    check_against_model(p, points, bins, what=f"path {path}, bins {bins}")


def test_pipeline_equals_the_host_engine_whatever_the_split(points):
    c = points
    own, cfg_filt = [("ret", "LessEqual", 2.0)], [("cls", "NotEqual", 5.0)]
    hists = lambda: [H.histogram(pcr, bins=37), H.histogram(pcr, bins=64, lo=0.0, hi=16.0, qs=[0.5], names=["low_median"], filt=own)]
    cpu = run(H.make_config(pcr, "cpu", hists(), cfg_filt=cfg_filt), [c], engine="host")
    whole = run(H.make_config(pcr, "gpu", hists(), cfg_filt=cfg_filt, result_location=DEVICE), [c], DEVICE)
    split = run(H.make_config(pcr, "gpu", hists(), cfg_filt=cfg_filt), [H.take(c, i) for i in H.uneven_splits(N, 7, 5)] +
                [H.take(c, np.arange(0))])
    back = run(H.make_config(pcr, "gpu", hists(), cfg_filt=cfg_filt), [H.take(c, np.arange(N)[::-1])])
    for p in (cpu, whole, split, back):
        p.finalize()
    assert whole.result().location() == DEVICE
    keep = H.keep_mask(c, cfg_filt)
    H.cubes_equal(cpu.histogram(0), H.cube(G, c["x"], c["y"], c["z"], LO, HI, 37, keep), "host engine against the model")
    H.cubes_equal(cpu.histogram(1), H.cube(G, c["x"], c["y"], c["z"], 0.0, 16.0, 64, keep & H.keep_mask(c, own)), "filtered histogram")
    names, ref = H.result_bands(cpu)
    assert names[2:] == [H.band_name("z", q) for q in QS] + ["low_median"]
    for p, what in ((whole, "device cloud, device result"), (split, "7 ingests"), (back, "reversed")):
        for i in range(2):
            H.cubes_equal(p.histogram(i), cpu.histogram(i), f"{what}: cube {i} against the host engine")
        for b, (u, w) in enumerate(zip(H.result_bands(p)[1][2:], ref[2:])):
            H.bits_equal(u, w, f"{what}: band {names[2 + b]} against the host engine")


def test_pipeline_filters_and_a_surface_channel(points):
    c = dict(points)
    surf = S.Surface(np.random.default_rng(2).integers(-3, 4, (20, 70)).astype(np.float32), G["min_x"] + 1.0, G["max_y"] - 1.0, 0.9, -0.8)
    surf.band[3, 5] = np.nan
    cfg_filt, own = [("cls", "NotEqual", 5.0)], [("ret", "LessEqual", 2.0), ("hag", "Greater", -2.5)]
    cfg = H.make_config(pcr, "gpu", [H.histogram(pcr, "hag", bins=37, filt=own)], cfg_filt=cfg_filt,
                        surface_channels=[pcr.SurfaceChannelConfig("hag", "z", pcr.SampleMode.Bilinear)])
    p = create(cfg)
    p.set_surface("hag", S.pcr_grid(pcr, surf))
    p.ingest(H.make_cloud(pcr, c, DEVICE))
    p.finalize()
    c["hag"] = S.model(surf, c["x"], c["y"], c["z"], S.BILINEAR)          # the model's own sampled channel
    check_against_model(p, c, 37, H.keep_mask(c, cfg_filt) & H.keep_mask(c, own), channel="hag", what="filters + hag")


def test_pipeline_band_placement_fill_ground_and_terrain(points):
    c = H.take(points, np.arange(0, N, 7))

    def cfg(mode, **kw):
        ground = pcr.GroundFilterConfig()
        ground.source_band, ground.top_band, ground.max_radius_cells = "z_2", "canopy", 2
        t = pcr.TerrainBandConfig()
        t.source_band, t.product = "median", pcr.TerrainProduct.Roughness
        return H.make_config(pcr, mode, [H.histogram(pcr, bins=37, qs=[0.5, 0.95], names=["median", "canopy"])], fill_nodata_radius=2,
                             ground=ground, terrain=[t], **kw)
    cpu = run(cfg("cpu"), [c], engine="host")
    gpu = run(cfg("gpu"), [c])
    dev = run(cfg("gpu", result_location=DEVICE), [c], DEVICE)
    for p in (cpu, gpu, dev):
        p.finalize()
    names, ref = H.result_bands(cpu)
    assert names == ["z_1", "z_2", "median", "canopy", "dtm", "hag", "median_roughness"]
    raw = H.percentiles(H.cube(G, c["x"], c["y"], c["z"], LO, HI, 37), LO, HI, 37, [0.5, 0.95])
    for p, what in ((gpu, "host result"), (dev, "device result")):
        got_names, got = H.result_bands(p)
        assert got_names == names
        for b in range(len(names)):
            H.bits_equal(got[b], ref[b], f"{what}: band {names[b]} against the host engine")
        for j in range(2):                                               # filled like a Max band: the raw cells stay
            m = ~np.isnan(raw[j])
            assert np.array_equal(H.bits(got[2 + j])[m], H.bits(raw[j])[m]) and np.isnan(got[2 + j]).sum() < np.isnan(raw[j]).sum()


def test_pipeline_finalize_twice_with_an_ingest_in_between(points):
    a, b = H.take(points, np.arange(0, N // 2)), H.take(points, np.arange(N // 2, N))
    p = run(H.make_config(pcr, "gpu", [H.histogram(pcr, bins=37)]), [a], DEVICE)
    p.finalize()
    check_against_model(p, a, 37, what="first finalize")
    p.ingest(H.make_cloud(pcr, b))
    p.finalize()
    check_against_model(p, points, 37, what="second finalize")


def test_pipeline_ingest_file_decodes_a_channel_only_the_histogram_names(tmp_path):
    fmt, n = 1, 6000
    rng = np.random.default_rng(9)
    f = LC.make_fields(fmt, n, rng)
    f["X"] = rng.integers(-500, 66_000, n).astype(np.int32)
    f["Y"] = rng.integers(-500, 19_000, n).astype(np.int32)
    f["Z"] = rng.integers(-100, 300, n).astype(np.int32)
    scale, offset = (0.001, 0.001, 0.125), (G["min_x"], G["min_y"], 0.0)
    path = str(tmp_path / "tile.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset)
    want = LC.expected(fmt, f, scale, offset, 0.0)
    cfg = H.make_config(pcr, "gpu", [H.histogram(pcr, bins=37)], reductions=(("intensity", "Count"), ("intensity", "Max")))
    p = create(cfg)
    assert p.ingest_file(path, 2500) == n
    p.finalize()
    c = dict(x=want["x"], y=want["y"], z=want["z"])
    check_against_model(p, c, 37, what="ingest_file")
    assert int(p.histogram(0).sum()) > n // 2


def test_a_budget_too_small_for_the_cube_refuses(points):
    small = 64 * G["W"] * G["H"] * 4                                     # room for the planes and bands, not for 256 bin planes
    ok = H.make_config(pcr, "gpu", [], gpu_memory_budget=small)
    assert not create(ok).out_of_core()
    cfg = H.make_config(pcr, "gpu", [H.histogram(pcr, bins=256)], gpu_memory_budget=small)
    assert pcr.Pipeline.create(cfg) is None
    assert "histograms are not supported on a pipeline that runs out of core" in pcr.pipeline_create_error()
    cfg.gpu_memory_budget = 0
    assert not create(cfg).out_of_core()


def test_checkpoints_are_refused_on_the_hip_engine(points, tmp_path):
    p = run(H.make_config(pcr, "gpu", [H.histogram(pcr)]), [points])
    for call in (p.save_state, p.load_state):
        with pytest.raises(RuntimeError, match="checkpoints do not carry the histograms"):
            call(str(tmp_path))


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_auto_path():
    W = 4096
    g = dict(min_x=0.0, min_y=0.0, max_x=float(W), max_y=float(W), cs=1.0, W=W, H=W, tw=4096, th=4096)
    n, bins, lo, hi = 10_000_000, 32, 0.0, 64.0
    rng = np.random.default_rng(33)
    x, y = rng.uniform(-8.0, W + 8.0, n), rng.uniform(-8.0, W + 8.0, n)
    z = (rng.standard_normal(n) * 12.0 + 30.0).astype(np.float32)
    z[rng.integers(0, n, 1000)] = np.nan
    cfg = H.make_config(pcr, "gpu", [H.histogram(pcr, lo=lo, hi=hi, bins=bins, qs=[0.5, 0.95])], g=g, reductions=(("z", "Count"),),
                        result_location=DEVICE)
    p = run(cfg, [dict(x=x, y=y, z=z)], DEVICE)
    assert p.last_scatter()["path"] == "binned"
    p.finalize()
    got = p.histogram(0)
    assert got.shape == (bins, W, W)
    valid, row, col = H.route(g, x, y)
    b = H.bin_of(z, lo, hi, bins)
    ok = valid & (b >= 0)
    assert int(got.sum(dtype=np.uint64)) == int(ok.sum())
    cells = rng.choice(W * W, 1000, replace=False)
    cell = row * W + col
    pick = ok & np.isin(cell, cells)
    slot = np.searchsorted(np.sort(cells), cell[pick])
    want = np.zeros((bins, 1000), np.uint32)
    np.add.at(want, (b[pick], slot), 1)
    rr, cc = np.sort(cells) // W, np.sort(cells) % W
    H.cubes_equal(got[:, rr, cc], want, "1 000 sampled cells")
    _, bands = H.result_bands(p)
    for j, wb in enumerate(H.percentiles(want[:, None, :], lo, hi, bins, [0.5, 0.95])):
        H.bits_equal(bands[1 + j][rr, cc], wb[0], "the sampled cells' bands")
