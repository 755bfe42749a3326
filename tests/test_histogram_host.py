"""Per-cell histograms (PipelineConfig::histograms) on the host engine and the C-ABI's host twin, against the NumPy model of
tests/histogram_common.py.  No GPU.  Every comparison is np.array_equal on uint32 views: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import histogram_common as H
import sample_grid_common as S
from conftest import load_cabi

pcr = pytest.importorskip("pcr")

G, QS, LO, HI = H.GRID, H.PERCENTILES, H.LO, H.HI
N = 20_000


@pytest.fixture(scope="module")
def points():
    return H.make_points(N, 11)


def run(cfg, clouds):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == "host"
    for c in clouds:
        p.ingest(H.make_cloud(pcr, c))
    return p


def check_against_model(p, c, bins, keep=None, channel="z", first_band=2, what=""):
    want = H.cube(G, c["x"], c["y"], c[channel], LO, HI, bins, keep)
    H.cubes_equal(p.histogram(0), want, what + " cube")
    names, bands = H.result_bands(p)
    for j, wb in enumerate(H.percentiles(want, LO, HI, bins, QS)):
        assert names[first_band + j] == H.band_name(channel, QS[j])
        H.bits_equal(bands[first_band + j], wb, f"{what} band {names[first_band + j]}")
    return want, names, bands


# ---- cube and bands against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 37, 256])
def test_cube_and_bands_match_the_model(points, bins):
    c = points
    z = c["z"]
    assert np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any() and (z < LO).any() and (z >= HI).any()
    assert (z == np.float32(HI)).any()
    valid, row, col = H.route(G, c["x"], c["y"])
    assert (~valid).any() and (c["x"] == G["min_x"]).any() and (c["y"] == G["max_y"]).any()
    assert np.bincount(row[valid] * G["W"] + col[valid]).max() >= 0.6 * N
    p = run(H.make_config(pcr, "cpu", [H.histogram(pcr, bins=bins)]), [c])
    H.cubes_equal(p.histogram(0), H.cube(G, c["x"], c["y"], z, LO, HI, bins), "before any finalize")     # pipe.histogram(i)
    p.finalize()
    want, names, bands = check_against_model(p, c, bins, what=f"bins {bins}")
    assert names[:2] == ["z_1", "z_2"] and len(names) == 2 + len(QS)
    assert int(want.sum()) == int((valid & ~np.isnan(z)).sum())           # out-of-range values and +-Inf are counted
    # monotone in q; a Max band is never below the last percentile's bin
    for a, b in zip(bands[2:-1], bands[3:]):
        m = ~np.isnan(a)
        assert (a[m] <= b[m]).all()


def test_values_on_bin_edges_land_in_the_upper_bin():
    bins, w = 256, (HI - LO) / 256                                       # 0.125: every edge is a float32
    edges = (LO + np.arange(bins) * w).astype(np.float32)
    c = dict(x=np.full(bins, G["min_x"] + 0.25), y=np.full(bins, G["max_y"] - 0.25), z=edges)
    p = run(H.make_config(pcr, "cpu", [H.histogram(pcr, bins=bins, qs=[])]), [c])
    got = p.histogram(0)
    assert (got[:, 0, 0] == 1).all() and int(got.sum()) == bins


# ---- splits, order, threads ---------------------------------------------------------------------------------------------------
def test_splits_order_and_threads_give_the_same_bits(points):
    c = points
    hist = lambda: [H.histogram(pcr, bins=37)]
    whole = run(H.make_config(pcr, "cpu", hist(), cpu_threads=1), [c])
    split = run(H.make_config(pcr, "cpu", hist(), cpu_threads=5), [H.take(c, idx) for idx in H.uneven_splits(N, 7, 5)])
    back = run(H.make_config(pcr, "cpu", hist(), cpu_threads=5), [H.take(c, np.arange(N)[::-1])])
    assert whole.host_threads() == 1 and split.host_threads() == 5
    for p in (whole, split, back):
        p.finalize()
    ref_cube = whole.histogram(0)
    _, ref = H.result_bands(whole)
    for p, what in ((split, "7 ingests, 5 threads"), (back, "reversed")):
        H.cubes_equal(p.histogram(0), ref_cube, what)
        for b, (u, w) in enumerate(zip(H.result_bands(p)[1][2:], ref[2:])):
            H.bits_equal(u, w, f"{what}: band {b}")


# ---- filters, a surface channel as the value ----------------------------------------------------------------------------------
def test_filters_and_a_surface_channel(points):
    c = dict(points)
    surf = S.Surface(np.random.default_rng(2).integers(-3, 4, (20, 70)).astype(np.float32), G["min_x"] + 1.0, G["max_y"] - 1.0, 0.9, -0.8)
    surf.band[3, 5] = np.nan
    cfg_filt, own = [("cls", "NotEqual", 5.0)], [("ret", "LessEqual", 2.0), ("hag", "Greater", -2.5)]
    cfg = H.make_config(pcr, "cpu", [H.histogram(pcr, "hag", bins=37, filt=own)], cfg_filt=cfg_filt,
                        surface_channels=[pcr.SurfaceChannelConfig("hag", "z", pcr.SampleMode.Bilinear)])
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    p.set_surface("hag", S.pcr_grid(pcr, surf))
    p.ingest(H.make_cloud(pcr, c))
    p.finalize()
    c["hag"] = S.model(surf, c["x"], c["y"], c["z"], S.BILINEAR)          # the model's own sampled channel
    keep = H.keep_mask(c, cfg_filt) & H.keep_mask(c, own)
    assert 0 < keep.sum() < N and np.isnan(c["hag"]).sum() > np.isnan(c["z"]).sum()
    check_against_model(p, c, 37, keep, channel="hag", what="filters + hag")


# ---- band placement -----------------------------------------------------------------------------------------------------------
def grid_of(band):
    d = pcr.BandDesc()
    d.name = "b"
    g = pcr.Grid.create(band.shape[1], band.shape[0], [d])
    g.set_band_array(0, band)
    return g


def test_bands_sit_behind_the_reductions_and_ahead_of_dtm_hag_terrain(points):
    c = H.take(points, np.arange(0, N, 7))                                # sparse: empty cells to fill
    ground = pcr.GroundFilterConfig()
    ground.source_band, ground.top_band, ground.max_radius_cells = "z_2", "canopy", 2
    t = pcr.TerrainBandConfig()
    t.source_band, t.product = "median", pcr.TerrainProduct.Roughness
    hist = H.histogram(pcr, bins=37, qs=[0.5, 0.95], names=["median", "canopy"])
    raw = run(H.make_config(pcr, "cpu", [H.histogram(pcr, bins=37, qs=[0.5, 0.95], names=["median", "canopy"])]), [c])
    p = run(H.make_config(pcr, "cpu", [hist], fill_nodata_radius=2, ground=ground, terrain=[t]), [c])
    raw.finalize()
    p.finalize()
    names, bands = H.result_bands(p)
    assert names == ["z_1", "z_2", "median", "canopy", "dtm", "hag", "median_roughness"]
    _, raw_bands = H.result_bands(raw)
    want = H.percentiles(H.cube(G, c["x"], c["y"], c["z"], LO, HI, 37), LO, HI, 37, [0.5, 0.95])
    for j in range(2):
        H.bits_equal(raw_bands[2 + j], want[j], "raw band")
        assert np.isnan(raw_bands[2 + j]).any()
        filled = pcr.fill_nodata(grid_of(raw_bands[2 + j]), 2)
        H.bits_equal(bands[2 + j], np.array(filled.band_array(0)), "filled like a Max band")
        assert np.isnan(bands[2 + j]).sum() < np.isnan(raw_bands[2 + j]).sum()
    # hag = top - dtm from the bands as they leave; the terrain band reads the filled median
    m = ~np.isnan(bands[5])
    assert m.any() and np.array_equal(bands[5][m], (bands[3] - bands[4])[m])
    assert (~np.isnan(bands[6])).any()


def test_finalize_twice_with_an_ingest_in_between(points):
    a, b = H.take(points, np.arange(0, N // 2)), H.take(points, np.arange(N // 2, N))
    p = run(H.make_config(pcr, "cpu", [H.histogram(pcr, bins=37)]), [a])
    p.finalize()
    check_against_model(p, a, 37, what="first finalize")
    p.ingest(H.make_cloud(pcr, b))
    p.finalize()
    check_against_model(p, points, 37, what="second finalize")


def test_an_empty_list_changes_nothing(points):
    with_h = run(H.make_config(pcr, "cpu", [H.histogram(pcr, bins=8, qs=[0.5])]), [points])
    without = run(H.make_config(pcr, "cpu", []), [points])
    with_h.finalize()
    without.finalize()
    n0, b0 = H.result_bands(without)
    n1, b1 = H.result_bands(with_h)
    assert n0 == ["z_1", "z_2"] and n1[:2] == n0
    for u, w in zip(b1, b0):
        H.bits_equal(u, w, "a reduction's band")
    with pytest.raises(RuntimeError, match="no histogram 0"):
        without.histogram(0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refused(histograms, match, **kw):
    assert pcr.Pipeline.create(H.make_config(pcr, "cpu", histograms, **kw)) is None
    assert match in pcr.pipeline_create_error(), pcr.pipeline_create_error()


def test_create_refuses_by_message():
    h = lambda **kw: H.histogram(pcr, **kw)
    refused([h() for _ in range(5)], "more than 4 histograms")
    refused([h(bins=0)], "bins must be between 1 and 256")
    refused([h(bins=257)], "bins must be between 1 and 256")
    refused([h(lo=float("nan"))], "finite bounds with lo < hi")
    refused([h(hi=float("inf"))], "finite bounds with lo < hi")
    refused([h(lo=3.0, hi=3.0)], "finite bounds with lo < hi")
    refused([h(qs=[0.5] * 17, names=[f"b{k}" for k in range(17)])], "more than 16 percentiles")
    refused([h(qs=[1.5])], "percentiles must lie in [0, 1]")
    refused([h(qs=[float("nan")])], "percentiles must lie in [0, 1]")
    refused([h(channel="")], "value_channel is empty")
    refused([h(qs=[0.5], names=["a", "b"])], "band_names is longer than percentiles")
    refused([h(qs=[0.5], names=["z_1"])], "collides with another band")                      # a reduction's band
    refused([h(qs=[0.5, 0.5])], "collides with another band")                               # its own twin
    refused([h(qs=[0.5]), h(qs=[0.5])], "collides with another band")                       # another histogram's
    ground = pcr.GroundFilterConfig()
    ground.source_band = "z_2"
    refused([h(qs=[0.5], names=["dtm"])], "collides with another band", ground=ground)
    t = pcr.TerrainBandConfig()
    t.source_band, t.product, t.band_name = "z_2", pcr.TerrainProduct.Hillshade, "shade"
    refused([h(qs=[0.5], names=["shade"])], "collides with another band", terrain=[t])
    refused([h()], "row-block shard", shard_row_begin=0, shard_row_end=16)
    # the filters join the plan of the reductions' filters and count against its limits
    nine = [h(qs=[], filt=[("ret", "Equal", float(k))]) for k in range(4)]
    cfg = H.make_config(pcr, "cpu", nine)
    specs = []
    for k in range(5):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "z", pcr.ReductionType.Count
        r.output_band_name = f"c{k}"
        r.filter.add("cls", pcr.CompareOp.Equal, float(k))
        specs.append(r)
    cfg.reductions = specs
    assert pcr.Pipeline.create(cfg) is None and "more than 8 distinct reduction filters" in pcr.pipeline_create_error()


def test_checkpoints_are_refused(points, tmp_path):
    p = run(H.make_config(pcr, "cpu", [H.histogram(pcr)]), [points])
    for call in (p.save_state, p.load_state):
        with pytest.raises(RuntimeError, match="checkpoints do not carry the histograms"):
            call(str(tmp_path))
    assert pcr.Pipeline.create(H.make_config(pcr, "cpu", [H.histogram(pcr)], resume=True, state_dir=str(tmp_path))) is None
    assert "checkpoints do not carry the histograms" in pcr.pipeline_create_error()


def test_a_bad_value_channel_leaves_no_state(points):
    p = run(H.make_config(pcr, "cpu", [H.histogram(pcr, "height", bins=8, qs=[0.5])]), [])
    with pytest.raises(RuntimeError, match="histogram value channel not found: height"):
        p.ingest(H.make_cloud(pcr, points))
    cloud = H.make_cloud(pcr, points)
    cloud.add_channel("height", pcr.DataType.Int32)
    with pytest.raises(RuntimeError, match="histogram value channel must be Float32"):
        p.ingest(cloud)
    assert int(p.histogram(0).sum()) == 0 and p.stats().points_processed == 0
    p.finalize()
    assert all(np.isnan(b).all() for b in H.result_bands(p)[1])


# ---- the percentile twin alone ------------------------------------------------------------------------------------------------
def twin(counts, lo, hi, qs):
    A = load_cabi()
    L = A.lib()
    bins, h, w = counts.shape
    g = A.make_grid((0, 0, w, h), dims=(w, h), tile=(w, h))
    outs = [np.full((h, w), -1.0, np.float32) for _ in qs]
    ptrs = (C.c_void_p * len(qs))(*[o.ctypes.data for o in outs])
    q = np.asarray(qs, np.float32)
    cc = np.ascontiguousarray(counts, np.uint32)
    wd = (np.float64(np.float32(hi)) - np.float64(np.float32(lo))) / bins
    rc = L.pcr_hip_histogram_percentiles_host(C.byref(g), cc.ctypes.data, bins, float(np.float32(lo)), float(wd), len(qs),
                                              q.ctypes.data, ptrs)
    assert rc == 0, L.pcr_hip_last_error()
    return outs


def test_percentile_twin_alone():
    bins = 8
    counts = np.zeros((bins, 2, 3), np.uint32)
    counts[3, 0, 0] = 1                                                  # a one-point cell: the bin's centre for every q
    counts[7, 0, 1] = 9                                                  # all points in the last bin
    counts[:, 0, 2] = [0, 2, 0, 0, 5, 0, 1, 0]
    counts[0, 1, 0] = 0xFFFFFFFF                                         # a counter at its limit
    counts[1, 1, 0] = 0xFFFFFFFF
    qs = [0.0, 1.0, 0.5, 0.3]
    got = twin(counts, 0.0, 16.0, qs)
    want = H.percentiles(counts, 0.0, 16.0, bins, qs)
    for u, w in zip(got, want):
        H.bits_equal(u, w, "twin against the model")
    for u in got:
        assert u[0, 0] == np.float32(7.0)                                # bin 3 of width 2: [6, 8)
        assert H.bits(u)[1, 1] == H.NAN_BITS and H.bits(u)[1, 2] == H.NAN_BITS          # empty cells
        assert 14.0 < u[0, 1] < 16.0
    assert got[0][0, 2] == np.float32(2.0 + 2.0 * 0.25) and got[1][0, 2] == np.float32(13.0)     # q = 0: rank 1 of 2 in [2, 4)
    assert got[0][0, 1] < got[3][0, 1] < got[2][0, 1] < got[1][0, 1]     # monotone in q inside one bin
    n16 = twin(counts, 0.0, 16.0, [k / 15.0 for k in range(16)])
    for u, w in zip(n16, H.percentiles(counts, 0.0, 16.0, bins, [k / 15.0 for k in range(16)])):
        H.bits_equal(u, w, "16 percentiles")


def test_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    g = A.make_grid((0, 0, 4, 4))
    counts = np.zeros((4, 4, 4), np.uint32)
    out = np.zeros((4, 4), np.float32)
    ptrs = (C.c_void_p * 1)(out.ctypes.data)
    q = np.array([0.5], np.float32)
    for fn, extra in ((L.pcr_hip_histogram_percentiles, (None,)), (L.pcr_hip_histogram_percentiles_host, ())):
        ok = (C.byref(g), counts.ctypes.data, 4, 0.0, 1.0, 1, q.ctypes.data, ptrs)
        for at, bad, msg in ((1, None, b"null argument"), (6, None, b"null argument"), (7, None, b"null argument"),
                             (2, 0, b"bins must be between 1 and 256"), (2, 257, b"bins must be between 1 and 256"),
                             (5, 0, b"between 1 and 16 percentiles"), (5, 17, b"between 1 and 16 percentiles")):
            args = list(ok)
            args[at] = bad
            assert fn(*args, *extra) == 1 and msg in L.pcr_hip_last_error(), (at, bad)
    assert L.pcr_hip_scatter_histogram(None, counts.ctypes.data, 4, 0.0, 1.0, None, None, None, 0) == 1
    assert b"null engine" in L.pcr_hip_last_error()
