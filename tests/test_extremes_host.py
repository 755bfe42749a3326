"""Per-cell extremes (PipelineConfig::extremes) on the host engine and the C-ABI's host twin, against the NumPy model of
tests/extremes_common.py.  No GPU.  Every comparison is np.array_equal on uint32 views: no tolerance anywhere.

One comparison needs a word.  "max_gap = +Inf equals the Min / Max band bit for bit": the contract folds -0.0 to +0.0 on the key,
so the extremes band never carries a -0.0, while a Min band keeps whichever zero fminf left.  The comparison therefore folds the
sign of a zero on the Min / Max band's bits (extremes_common.fold_zero) -- the contract's own fold, nothing wider -- and asserts
separately that the extremes band holds no -0.0."""
import ctypes as C

import numpy as np
import pytest

import extremes_common as E
import sample_grid_common as S
from conftest import load_cabi

pcr = pytest.importorskip("pcr")

G = E.GRID
N = 20_000
INF = float("inf")
GAPS = [0.0, 1.0, INF]
LOWEST, HIGHEST = E.LOWEST, E.HIGHEST


@pytest.fixture(scope="module")
def points():
    c = E.make_points(N, 11)
    E.check_cloud(c, G)
    return c


def run(cfg, clouds):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == "host"
    for c in clouds:
        p.ingest(E.make_cloud(pcr, c))
    return p


def three_gaps(k, side, **kw):
    return [E.entry(pcr, "z", side, k, gap, name=f"g{j}", **kw) for j, gap in enumerate(GAPS)]


# ---- planes and bands against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [LOWEST, HIGHEST], ids=["lowest", "highest"])
@pytest.mark.parametrize("k", [2, 4, 8])
def test_values_and_bands_match_the_model(points, k, side):
    c = points
    want = E.planes(G, c["x"], c["y"], c["z"], k, side)
    assert ((want != E.EMPTY).sum(axis=0) == k).mean() > 0.5             # most cells saw k distinct values or more
    p = run(E.make_config(pcr, "cpu", three_gaps(k, side)), [c])
    for i in range(3):                                                    # pipe.extremes(i) before any finalize
        got = p.extremes(i)
        assert got.dtype == np.float32 and got.shape == (k, G["H"], G["W"])
        E.bits_equal(got, E.value_of(want, side), f"k {k}, side {side}: values of entry {i} before any finalize")
    p.finalize()
    names, bands = E.result_bands(p)
    assert names == ["z_1", "z_2", "g0", "g1", "g2"]
    for j, gap in enumerate(GAPS):
        E.bits_equal(bands[2 + j], E.band(want, side, gap), f"k {k}, side {side}, max_gap {gap}")
        assert not (E.bits(bands[2 + j]) == 0x80000000).any()             # -0.0 is folded
    # max_gap = +Inf is the plain Min / Max: bit for bit wherever that band is not NaN (a zero's sign folded: module docstring)
    plain = bands[1] if side == LOWEST else bands[0]
    m = ~np.isnan(plain)
    assert m.any() and np.array_equal(E.fold_zero(plain)[m], E.bits(bands[4])[m])
    # (a cell whose only values are +Inf (Lowest) has no Min -- the fold never leaves its identity -- but has an extreme)
    assert not (np.isnan(bands[4]) & m).any() and np.isinf(bands[4][~m & ~np.isnan(bands[4])]).all()
    # the gaps matter: 0 steps over every distinct value it kept, 1 over none of the quantised ones
    assert (E.bits(bands[2]) != E.bits(bands[4])).any()


def test_the_kth_value_when_every_gap_is_too_wide():
    """Documented: a cell whose k kept values are all more than max_gap apart yields the k-th."""
    z = np.array([5.0, 1.0, 9.0, 3.0, 7.0, 1.0], np.float32)
    c = dict(x=np.full(6, G["min_x"] + 0.25), y=np.full(6, G["max_y"] - 0.25), z=z)
    p = run(E.make_config(pcr, "cpu", [E.entry(pcr, "z", LOWEST, 3, 1.0), E.entry(pcr, "z", HIGHEST, 4, 1.5)]), [c])
    assert p.extremes(0)[:, 0, 0].tolist() == [1.0, 3.0, 5.0] and p.extremes(1)[:, 0, 0].tolist() == [9.0, 7.0, 5.0, 3.0]
    p.finalize()
    names, bands = E.result_bands(p)
    assert names[2:] == ["z_low", "z_high"]
    assert bands[2][0, 0] == 5.0 and bands[3][0, 0] == 3.0
    assert np.isnan(bands[2][1, 1]) and E.bits(bands[2])[1, 1] == E.NAN_BITS


# ---- splits, order, threads ---------------------------------------------------------------------------------------------------
def test_splits_order_and_threads_give_the_same_bits(points):
    c = points
    ext = lambda: [E.entry(pcr, "z", LOWEST, 4, 1.0), E.entry(pcr, "z", HIGHEST, 8, 0.25)]
    whole = run(E.make_config(pcr, "cpu", ext(), cpu_threads=1), [c])
    split = run(E.make_config(pcr, "cpu", ext(), cpu_threads=5), [E.take(c, idx) for idx in E.uneven_splits(N, 7, 5)])
    back = run(E.make_config(pcr, "cpu", ext(), cpu_threads=5), [E.take(c, np.arange(N)[::-1])])
    assert whole.host_threads() == 1 and split.host_threads() == 5
    for p in (whole, split, back):
        p.finalize()
    E.bits_equal(whole.extremes(0), E.value_of(E.planes(G, c["x"], c["y"], c["z"], 4, LOWEST), LOWEST), "1 thread against the model")
    _, ref = E.result_bands(whole)
    for p, what in ((split, "7 ingests, 5 threads"), (back, "reversed")):
        for i in range(2):
            E.bits_equal(p.extremes(i), whole.extremes(i), f"{what}: values {i}")
        for b, (u, w) in enumerate(zip(E.result_bands(p)[1][2:], ref[2:])):
            E.bits_equal(u, w, f"{what}: band {b}")


# ---- filters, a surface channel as the value ----------------------------------------------------------------------------------
def test_filters_and_a_surface_channel(points):
    c = dict(points)
    surf = S.Surface(np.random.default_rng(2).integers(-3, 4, (20, 70)).astype(np.float32), G["min_x"] + 1.0, G["max_y"] - 1.0, 0.9, -0.8)
    surf.band[3, 5] = np.nan
    cfg_filt, own = [("cls", "NotEqual", 5.0)], [("ret", "LessEqual", 2.0), ("hag", "Greater", -2.5)]
    cfg = E.make_config(pcr, "cpu", [E.entry(pcr, "hag", HIGHEST, 4, 0.5, filt=own)], cfg_filt=cfg_filt,
                        surface_channels=[pcr.SurfaceChannelConfig("hag", "z", pcr.SampleMode.Bilinear)])
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    p.set_surface("hag", S.pcr_grid(pcr, surf))
    p.ingest(E.make_cloud(pcr, c))
    p.finalize()
    c["hag"] = S.model(surf, c["x"], c["y"], c["z"], S.BILINEAR)          # the model's own sampled channel
    keep = E.keep_mask(c, cfg_filt) & E.keep_mask(c, own)
    assert 0 < keep.sum() < N and np.isnan(c["hag"]).sum() > np.isnan(c["z"]).sum()
    want = E.planes(G, c["x"], c["y"], c["hag"], 4, HIGHEST, keep)
    E.bits_equal(p.extremes(0), E.value_of(want, HIGHEST), "filters + hag: values")
    names, bands = E.result_bands(p)
    assert names[2] == "hag_high"
    E.bits_equal(bands[2], E.band(want, HIGHEST, 0.5), "filters + hag: band")


# ---- band placement -----------------------------------------------------------------------------------------------------------
def grid_of(band):
    d = pcr.BandDesc()
    d.name = "b"
    g = pcr.Grid.create(band.shape[1], band.shape[0], [d])
    g.set_band_array(0, band)
    return g


def test_bands_sit_behind_the_percentiles_and_ahead_of_dtm_hag_terrain(points):
    import histogram_common as H
    c = E.take(points, np.arange(0, N, 7))                                # sparse: empty cells to fill
    c["z"] = np.where(np.isinf(c["z"]), np.float32(0.5), c["z"])          # (an infinite ground says nothing about the fill)

    def cfg(**kw):
        ground = pcr.GroundFilterConfig()
        ground.source_band, ground.top_band, ground.max_radius_cells = "z_low", "z_high", 2
        t = pcr.TerrainBandConfig()
        t.source_band, t.product = "z_low", pcr.TerrainProduct.Roughness
        out = E.make_config(pcr, "cpu", [E.entry(pcr, "z", LOWEST, 4, 1.0), E.entry(pcr, "z", HIGHEST, 2, 0.0)], **kw)
        out.histograms = [H.histogram(pcr, bins=8, qs=[0.5], names=["median"])]
        if kw:
            out.ground, out.terrain = ground, [t]
        return out
    raw = run(cfg(), [c])
    p = run(cfg(fill_nodata_radius=2), [c])
    raw.finalize()
    p.finalize()
    names, bands = E.result_bands(p)
    assert names == ["z_1", "z_2", "median", "z_low", "z_high", "dtm", "hag", "z_low_roughness"]
    raw_names, raw_bands = E.result_bands(raw)
    assert raw_names == names[:5]
    for b, (side, k, gap) in ((3, (LOWEST, 4, 1.0)), (4, (HIGHEST, 2, 0.0))):
        E.bits_equal(raw_bands[b], E.band(E.planes(G, c["x"], c["y"], c["z"], k, side), side, gap), "raw band")
        assert np.isnan(raw_bands[b]).any()
        filled = pcr.fill_nodata(grid_of(raw_bands[b]), 2)                 # (Min and Max bands are filled by the same rule)
        E.bits_equal(bands[b], np.array(filled.band_array(0)), "filled like a Min / Max band")
        assert np.isnan(bands[b]).sum() < np.isnan(raw_bands[b]).sum()
    # the ground filter read z_low: its DTM is what the stand-alone filter makes of the raw band, filled
    spec = pcr.GroundFilterSpec()
    spec.max_radius_cells = 2
    dtm = pcr.ground_filter(grid_of(raw_bands[3]), 0, spec, G["cs"])
    E.bits_equal(bands[5], np.array(pcr.fill_nodata(dtm, 2).band_array(0)), "dtm from z_low")
    m = ~np.isnan(bands[6])
    assert m.any() and np.array_equal(bands[6][m], (bands[4] - bands[5])[m])          # hag = top - dtm as they leave
    assert (~np.isnan(bands[7])).any()                                                 # the terrain band read the filled z_low


def test_finalize_twice_with_an_ingest_in_between(points):
    a, b = E.take(points, np.arange(0, N // 2)), E.take(points, np.arange(N // 2, N))
    b = dict(b, z=(b["z"] - np.float32(1.25)).astype(np.float32))          # lower values: slots are displaced
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    p = run(E.make_config(pcr, "cpu", [E.entry(pcr, "z", LOWEST, 4, 0.25)]), [a])
    p.finalize()
    E.bits_equal(E.result_bands(p)[1][2], E.band(E.planes(G, a["x"], a["y"], a["z"], 4, LOWEST), LOWEST, 0.25), "first finalize")
    p.ingest(E.make_cloud(pcr, b))
    p.finalize()
    want = E.planes(G, both["x"], both["y"], both["z"], 4, LOWEST)
    E.bits_equal(p.extremes(0), E.value_of(want, LOWEST), "second finalize: values")
    E.bits_equal(E.result_bands(p)[1][2], E.band(want, LOWEST, 0.25), "second finalize")


def test_an_empty_list_changes_nothing(points):
    with_e = run(E.make_config(pcr, "cpu", [E.entry(pcr)]), [points])
    without = run(E.make_config(pcr, "cpu", []), [points])
    with_e.finalize()
    without.finalize()
    n0, b0 = E.result_bands(without)
    n1, b1 = E.result_bands(with_e)
    assert n0 == ["z_1", "z_2"] and n1 == n0 + ["z_low"]
    for u, w in zip(b1, b0):
        E.bits_equal(u, w, "a reduction's band")
    with pytest.raises(RuntimeError, match="no extremes entry 0"):
        without.extremes(0)


# ---- the scenario that shows the point ----------------------------------------------------------------------------------------
def test_pits_and_birds_on_a_tilted_plane():
    def make(cfg, c):
        p = run(cfg, [c])
        p.finalize()
        return p
    E.check_scene(pcr, make)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refused(extremes, match, **kw):
    assert pcr.Pipeline.create(E.make_config(pcr, "cpu", extremes, **kw)) is None
    assert match in pcr.pipeline_create_error(), pcr.pipeline_create_error()


def test_create_refuses_by_message():
    e = lambda **kw: E.entry(pcr, **kw)
    refused([e(name=f"b{j}") for j in range(5)], "more than 4 extremes entries")
    refused([e(k=1)], "k must be between 2 and 8")
    refused([e(k=9)], "k must be between 2 and 8")
    refused([e(max_gap=-0.5)], "max_gap must not be negative or NaN")
    refused([e(max_gap=float("nan"))], "max_gap must not be negative or NaN")
    refused([e(channel="")], "value_channel is empty")
    odd = e()
    odd.side = 7
    refused([odd], "side is neither Lowest nor Highest")
    refused([e(name="z_1")], "collides with another band")                                   # a reduction's band
    refused([e(), e()], "collides with another band")                                        # its own twin
    ground = pcr.GroundFilterConfig()
    ground.source_band = "z_2"
    refused([e(name="dtm")], "collides with another band", ground=ground)
    t = pcr.TerrainBandConfig()
    t.source_band, t.product, t.band_name = "z_2", pcr.TerrainProduct.Hillshade, "shade"
    refused([e(name="shade")], "collides with another band", terrain=[t])
    import histogram_common as H
    cfg = E.make_config(pcr, "cpu", [e(name="median")])
    cfg.histograms = [H.histogram(pcr, bins=8, qs=[0.5], names=["median"])]
    assert pcr.Pipeline.create(cfg) is None and "collides with another band" in pcr.pipeline_create_error()
    refused([e()], "extremes are not supported on a row-block shard", shard_row_begin=0, shard_row_end=16)
    # the filters join the plan of the reductions' filters and count against its limits
    four = [e(name=f"b{j}", filt=[("ret", "Equal", float(j))]) for j in range(4)]
    cfg = E.make_config(pcr, "cpu", four)
    specs = []
    for j in range(5):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "z", pcr.ReductionType.Count
        r.output_band_name = f"c{j}"
        r.filter.add("cls", pcr.CompareOp.Equal, float(j))
        specs.append(r)
    cfg.reductions = specs
    assert pcr.Pipeline.create(cfg) is None and "more than 8 distinct reduction filters" in pcr.pipeline_create_error()


def test_checkpoints_are_refused(points, tmp_path):
    p = run(E.make_config(pcr, "cpu", [E.entry(pcr)]), [points])
    for call in (p.save_state, p.load_state):
        with pytest.raises(RuntimeError, match="checkpoints do not carry the extremes"):
            call(str(tmp_path))
    assert pcr.Pipeline.create(E.make_config(pcr, "cpu", [E.entry(pcr)], resume=True, state_dir=str(tmp_path))) is None
    assert "checkpoints do not carry the extremes" in pcr.pipeline_create_error()


def test_a_bad_value_channel_leaves_no_state(points):
    p = run(E.make_config(pcr, "cpu", [E.entry(pcr, "height")]), [])
    with pytest.raises(RuntimeError, match="extremes value channel not found: height"):
        p.ingest(E.make_cloud(pcr, points))
    cloud = E.make_cloud(pcr, points)
    cloud.add_channel("height", pcr.DataType.Int32)
    with pytest.raises(RuntimeError, match="extremes value channel must be Float32"):
        p.ingest(cloud)
    assert np.isnan(p.extremes(0)).all() and p.stats().points_processed == 0
    p.finalize()
    assert all(np.isnan(b).all() for b in E.result_bands(p)[1])


# ---- the twin alone -----------------------------------------------------------------------------------------------------------
def twin(keys, side, max_gap, own=None):
    A = load_cabi()
    L = A.lib()
    k, h, w = keys.shape
    g = A.make_grid((0, 0, w, h), dims=(w, h), tile=(w, h))
    r0, r1 = own if own else (0, h)
    g.own_row0, g.own_row1 = r0, r1
    out = np.full((r1 - r0, w), -1.0, np.float32)
    vals = np.full((k, r1 - r0, w), -1.0, np.float32)
    kk = np.ascontiguousarray(keys, np.uint32)
    rc = L.pcr_hip_extremes_band_host(C.byref(g), kk.ctypes.data, k, side, C.c_float(max_gap), out.ctypes.data, vals.ctypes.data)
    assert rc == 0, L.pcr_hip_last_error()
    return out, vals


def test_band_twin_alone():
    z = lambda *v: E.key_of(np.array(v, np.float32), LOWEST)
    k = 4
    keys = np.full((k, 2, 3), E.EMPTY, np.uint32)
    keys[:1, 0, 0] = z(2.5)                                              # one value
    keys[:4, 0, 1] = z(-60.0, -58.5, 1.0, 1.5)                           # two outliers 1.5 apart, then the ground
    keys[:3, 0, 2] = z(-np.inf, -0.0, 0.5)                               # -Inf is a value; the zero is +0.0
    keys[:4, 1, 0] = z(0.0, 2.0, 4.0, 6.0)                               # every gap too wide: the k-th
    keys[:2, 1, 1] = z(3.0, np.inf)
    for gap in (0.0, 1.0, 1.5, INF):
        out, vals = twin(keys, LOWEST, gap)
        E.bits_equal(out, E.band(keys, LOWEST, gap), f"twin against the model, max_gap {gap}")
        E.bits_equal(vals, E.value_of(keys, LOWEST), "decoded values")
    out, _ = twin(keys, LOWEST, 1.0)
    assert out[0].tolist() == [2.5, 1.0, 0.0] and E.bits(out)[0, 2] == 0 and out[1, 0] == 6.0 and out[1, 1] == np.inf
    assert E.bits(out)[1, 2] == E.NAN_BITS
    assert twin(keys, LOWEST, 1.5)[0][0, 1] == -60.0                      # a gap equal to max_gap is not stepped over
    hk = np.full((2, 1, 2), E.EMPTY, np.uint32)
    hk[:, 0, 0] = E.key_of(np.array([180.0, 21.0], np.float32), HIGHEST)
    out, vals = twin(hk, HIGHEST, 1.0)
    assert out[0, 0] == 21.0 and vals[:, 0, 0].tolist() == [180.0, 21.0] and E.bits(out)[0, 1] == E.NAN_BITS
    E.bits_equal(out, E.band(hk, HIGHEST, 1.0), "highest")
    out, vals = twin(keys, LOWEST, 1.0, own=(1, 2))                       # the owned rows alone
    E.bits_equal(out, E.band(keys, LOWEST, 1.0)[1:2], "owned rows")
    E.bits_equal(vals, E.value_of(keys, LOWEST)[:, 1:2], "owned rows: values")


def test_key_range():
    v = np.array([-np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4e38, np.inf], np.float32)
    for side in (LOWEST, HIGHEST):
        key = E.key_of(v, side).astype(np.int64)
        assert key.min() == 0x007FFFFF and key.max() == 0xFF800000 and key[4] == key[5] == (0x80000000 if side == LOWEST else 0x7FFFFFFF)
        d = np.diff(key)
        assert ((d >= 0) if side == LOWEST else (d <= 0)).all() and (d != 0).sum() == 8
        assert np.array_equal(E.value_of(E.key_of(v, side), side)[[0, 2, 7, 9]], v[[0, 2, 7, 9]])
    assert E.key_of(np.array([np.nan], np.float32), LOWEST)[0] == E.EMPTY


def test_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    g = A.make_grid((0, 0, 4, 4))
    keys = np.full((4, 4, 4), E.EMPTY, np.uint32)
    out = np.zeros((4, 4), np.float32)
    for fn, extra in ((L.pcr_hip_extremes_band, (None, None)), (L.pcr_hip_extremes_band_host, (None,))):
        ok = [C.byref(g), keys.ctypes.data, 4, 0, C.c_float(1.0), out.ctypes.data]
        for at, bad, msg in ((1, None, b"null argument"), (5, None, b"null argument"), (2, 1, b"k must be between 2 and 8"),
                             (2, 9, b"k must be between 2 and 8"), (3, 2, b"side must be 0 (lowest) or 1 (highest)"),
                             (4, C.c_float(-1.0), b"max_gap must not be negative or NaN"),
                             (4, C.c_float(float("nan")), b"max_gap must not be negative or NaN")):
            args = list(ok)
            args[at] = bad
            assert fn(*args, *extra) == 1 and msg in L.pcr_hip_last_error(), (at, bad)
    assert L.pcr_hip_scatter_extremes(None, keys.ctypes.data, 4, 0, None, None, None, 0) == 1
    assert b"null engine" in L.pcr_hip_last_error()
