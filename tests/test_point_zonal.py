"""Point zonal tables on the host: the C-ABI's host twins (pcr_hip_point_fold_*_host) held BIT FOR BIT to the model of the
contract in tests/point_zonal_common.py -- every way labels can lie, labels at the table's and the format's edges, mask bytes
0, 1, 255 and none, values at the step clamp, tables that wrap, the info words, n = 0 -- every argument error, and the host
engine's PipelineConfig.point_zonal: the table against the model, chunked ingests, finalize, refusals, the per-cell table it
must equal when every point lies in its own cell's zone, and the plot whose count the cell-resolution route gets wrong."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pcr
import point_zonal_common as P
import zonal_common as ZC
from conftest import load_cabi

F32, U8, U32, I64, U64 = np.float32, np.uint8, np.uint32, np.int64, np.uint64
CPU = pcr.ExecutionMode.CPU
N = 1337                                     # points of the twin tests: 20 waves and a ragged one
ZCAP = 9                                     # their table's capacity (the patterns use zones 1..7, Z and Z + 1)


@pytest.fixture(scope="module")
def A():
    return load_cabi()


# ---- 1: the host twins against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_stats_twin_equals_the_model(A, masked):
    values = P.values_for(N)
    mask = P.masks_for(N) if masked else None
    for name, labels in P.label_patterns(N, ZCAP).items():
        want = P.fold(labels, mask, values, ZCAP, stat=(0.0, 100.0))
        got = P.run_fold_stats(A, False, labels, mask, values, ZCAP)
        P.same(got, want, f"{name} masked {masked}")
    labels = P.label_patterns(N, ZCAP)["edge labels scattered in"]
    want = P.fold(labels, mask, values, ZCAP, stat=(0.0, 100.0))
    assert want["info"][1] > 0 and want["info"][0] == ZCAP                 # Z + 1 and 2^24 overflow, Z itself is a row
    only = P.run_fold_stats(A, False, labels, mask, None, ZCAP)
    P.same(only, dict(points=want["points"], info=want["info"]), "points alone")
    none = P.run_fold_stats(A, False, labels, mask, values, ZCAP, points=False, info=None)
    P.same(none, {k: want[k] for k in ("n", "s1", "s2")}, "no points, no info")


def test_values_at_the_clamp_and_negative_sums(A):
    origin, inv_res = 1.5, 8.0
    res = 1.0 / inv_res
    vals = np.array([origin + P.Q * res, origin + (P.Q - 1) * res, origin - P.Q * res, origin - (P.Q - 1) * res, np.inf, -np.inf,
                     np.nan, origin - 3 * res, origin - 5 * res, 1e30, -1e30], F32)
    assert [P.step_of(v, origin, inv_res) for v in vals] == [P.Q, P.Q - 1, -P.Q, -P.Q + 1, P.Q, -P.Q, None, -3, -5, P.Q, -P.Q]
    labels = np.array([1, 1, 2, 2, 1, 2, 1, 3, 3, 1, 2], F32)
    want = P.fold(labels, None, vals, 3, stat=(origin, inv_res))
    assert want["points"].tolist() == [5, 4, 2] and want["n"].tolist() == [4, 4, 2] and want["s1"].tolist()[1:] == [-4 * P.Q + 1, -8]
    P.same(P.run_fold_stats(A, False, labels, None, vals, 3, origin, inv_res), want, "clamp")


def test_tables_that_wrap_and_accumulate(A):
    values = P.values_for(N)
    mask = P.masks_for(N)
    labels = P.label_patterns(N, ZCAP)["runs of 65"]
    want = P.fold(labels, mask, values, ZCAP, stat=(0.0, 100.0), seed=P.SEED, info=(3, P.SEED))
    assert int(want["points"][0]) < 1000 and int(want["s2"][0]) < (1 << 63) and int(want["info"][1]) == P.SEED      # wrapped
    got = P.run_fold_stats(A, False, labels, mask, values, ZCAP, seed=P.SEED, info=(3, P.SEED))
    P.same(got, want, "seeded")
    once = P.fold(labels, mask, values, ZCAP, stat=(0.0, 100.0))
    for calls in (3, 7):                                                     # the tables accumulate across calls
        P.same(P.run_fold_stats(A, False, labels, mask, values, ZCAP, calls=calls), once, f"{calls} calls")
    high = P.run_fold_stats(A, False, labels, mask, values, ZCAP, info=(8, 0))
    assert high["info"].tolist() == [8, 0]                                   # info[0] is a running maximum


@pytest.mark.parametrize("bins", [1, 63, 64, 65, 256])
def test_hist_twin_equals_the_model(A, bins):
    values = P.values_for(N)
    mask = P.masks_for(N)
    lo, inv_w = -3.0, bins / 64.0
    for name in ("one zone", "runs of 63", "edge labels scattered in", "shuffled"):
        labels = P.label_patterns(N, ZCAP)[name]
        for msk, seed in ((None, 0), (mask, P.SEED)):
            want = P.fold(labels, msk, values, ZCAP, hist=(bins, lo, inv_w), seed=seed)
            got = P.run_fold_hist(A, False, labels, msk, values, ZCAP, bins, lo, inv_w, seed=seed)
            P.same(got, dict(counts=want["counts"], info=want["info"]), f"bins {bins} {name}")


def test_labels_at_the_edges_of_the_format(A):
    labels = np.array([float(2 ** 24), float(2 ** 24 + 2), float(2 ** 24 - 1), 1.0, 0.0, -0.0, -1.0, 2.5, np.nan, np.inf, -np.inf], F32)
    vals = np.arange(len(labels)).astype(F32)
    full = P.run_fold_stats(A, False, labels, None, None, 2 ** 24)       # (`points` alone: one table of 128 MB)
    assert full["points"][2 ** 24 - 1] == 1 and full["points"][2 ** 24 - 2] == 1 and full["points"][0] == 1
    assert int(full["points"].sum()) == 3 and full["info"].tolist() == [2 ** 24, 0]
    small = P.run_fold_stats(A, False, labels, None, vals, 1)
    assert small["points"].tolist() == [1] and small["info"].tolist() == [1, 2]          # 2^24 and 2^24 - 1 overflow a table of one row
    masked = P.run_fold_stats(A, False, labels, np.array([0, 1, 0] + [1] * 8, U8), vals, 1)
    assert masked["info"].tolist() == [1, 0]                                             # a masked point overflows nothing


def test_no_point_changes_nothing(A):
    got = P.run_fold_stats(A, False, np.zeros(0, F32), None, np.zeros(0, F32), 4, seed=77, info=(2, 5))
    assert all(got[k].tolist() == [77] * 4 for k in ("points", "n", "s1", "s2")) and got["info"].tolist() == [2, 5]
    got = P.run_fold_hist(A, False, np.zeros(0, F32), None, np.zeros(0, F32), 4, 3, seed=77, info=(2, 5))
    assert (got["counts"] == 77).all() and got["info"].tolist() == [2, 5]


# ---- 2: every argument error ---------------------------------------------------------------------------------------------------
def test_argument_errors(A):
    L = A.lib()
    n = 16
    lab, val, msk = np.ones(n, F32), np.ones(n, F32), np.ones(n, U8)
    t = [np.zeros(8, U64) for _ in range(4)]
    info = np.zeros(2, U64)
    zc = np.zeros(8 * 4, U64)
    p = lambda a: a.ctypes.data
    prm = A.PointFoldParams(0, 0)

    def stats(lab_p=p(lab), msk_p=p(msk), val_p=p(val), n=n, origin=0.0, inv_res=100.0, Z=8, prm_p=C.byref(prm), pts=p(t[0]), a=p(t[1]),
              b=p(t[2]), d=p(t[3]), inf=p(info)):
        return L.pcr_hip_point_fold_stats_host(lab_p, msk_p, val_p, n, origin, inv_res, Z, prm_p, pts, a, b, d, inf)

    def hist(lab_p=p(lab), msk_p=p(msk), val_p=p(val), n=n, bins=4, lo=0.0, inv_w=1.0, Z=8, prm_p=C.byref(prm), z_p=p(zc), inf=p(info)):
        return L.pcr_hip_point_fold_hist_host(lab_p, msk_p, val_p, n, bins, lo, inv_w, Z, prm_p, z_p, inf)

    assert stats() == 0 and hist() == 0
    assert stats(msk_p=None, inf=None) == 0 and stats(val_p=None, a=None, b=None, d=None) == 0 and stats(pts=None) == 0
    path3, path2, blocks = A.PointFoldParams(3, 0), A.PointFoldParams(2, 0), A.PointFoldParams(0, -1)
    cap_s = A.POINT_FOLD_LDS_BYTES // A.POINT_FOLD_STATS_ROW_BYTES
    for kw, msg in ((dict(lab_p=None), "null argument"), (dict(prm_p=None), "null argument"), (dict(val_p=None), "null argument"),
                    (dict(b=None), "null argument"), (dict(val_p=None, a=None, b=None, d=None, pts=None), "null argument"),
                    (dict(Z=0), "Z must be between 1 and 2^24"), (dict(Z=2 ** 24 + 1), "Z must be between 1 and 2^24"),
                    (dict(origin=float("nan")), "origin and inv_res must be finite"), (dict(inv_res=float("inf")), "origin and inv_res must be finite"),
                    (dict(inv_res=0.0), "inv_res positive"), (dict(prm_p=C.byref(path3)), "path must be 0 (auto), 1 (global atomics) or 2 (LDS table)"),
                    (dict(prm_p=C.byref(path2), Z=cap_s + 1), f"path 2 holds at most {cap_s} zones"),
                    (dict(prm_p=C.byref(blocks)), "blocks must be between 0 (auto) and 65536"),
                    (dict(n=2 ** 40 + 1), "more than 2^40 points"),
                    (dict(pts=p(lab)), "a table overlaps an input"), (dict(a=p(val) + 8), "a table overlaps an input"),
                    (dict(inf=p(msk)), "a table overlaps an input"), (dict(d=p(t[0])), "two tables overlap"),
                    (dict(inf=p(t[1]) + 8), "two tables overlap")):
        assert stats(**kw) != 0, kw
        assert msg in L.pcr_hip_last_error().decode(), (kw, L.pcr_hip_last_error())
    cap_h = A.POINT_FOLD_LDS_BYTES // (4 * 4)
    for kw, msg in ((dict(lab_p=None), "null argument"), (dict(val_p=None), "null argument"), (dict(z_p=None), "null argument"),
                    (dict(prm_p=None), "null argument"), (dict(bins=0), "bins must be between 1 and 256"),
                    (dict(bins=257), "bins must be between 1 and 256"), (dict(Z=0), "Z must be between 1 and 2^24"),
                    (dict(lo=float("inf")), "lo and inv_w must be finite"), (dict(inv_w=-1.0), "inv_w positive"),
                    (dict(prm_p=C.byref(path3)), "path must be 0"), (dict(prm_p=C.byref(path2), Z=cap_h + 1), f"path 2 holds at most {cap_h} zones"),
                    (dict(z_p=p(val)), "a table overlaps an input"), (dict(inf=p(zc) + 16), "two tables overlap")):
        assert hist(**kw) != 0, kw
        assert msg in L.pcr_hip_last_error().decode(), (kw, L.pcr_hip_last_error())
    assert stats(prm_p=C.byref(path2), Z=8) == 0                             # (a twin takes any path that fits: it has one loop)


# ---- 3: the host engine's PipelineConfig.point_zonal ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plot_case():
    """The plots, 3000 dyadic points over and a little beyond the grid, their exact labels, and the model's table under the
    pipeline filter and the specs' own."""
    import points_in_polygons_common as PP
    polys = PP.plots()
    c = PP.plot_points(3000, 21)
    labels = PP.model(polys, c["x"], c["y"])
    want, counts = P.pipeline_model(c, labels, 64, P.CFG_FILT, P.STAT_FILT, P.HIST_FILT)
    outside = (c["x"] < 0) | (c["x"] > 40) | (c["y"] < 0) | (c["y"] > 24)
    assert int((outside & (labels >= 1)).sum()) > 5                        # points outside the grid but inside a plot: they count
    return polys, c, labels, want, counts


def filtered_pipeline(polys):
    p = P.plot_pipeline(pcr, "cpu", P.CFG_FILT, stat_filt=P.STAT_FILT, hist_filt=P.HIST_FILT)
    p.set_polygons("plot", polys.to_pcr())
    return p


@pytest.mark.parametrize("chunks", [1, 3, 7])
def test_pipeline_equals_the_model(plot_case, chunks):
    import sample_grid_common as SG
    polys, c, labels, want, counts = plot_case
    p = filtered_pipeline(polys)
    empty = p.point_zonal(0)
    assert list(empty) == list(want) and all(len(v) == 0 for v in empty.values())           # before the first ingest: no row
    n = len(c["x"])
    for k in range(chunks):
        p.ingest(SG.dict_cloud(pcr, P.piece(c, n * k // chunks, n * (k + 1) // chunks)))
    got = p.point_zonal(0)
    assert list(got) == ["zone", "points", "z_n", "z_mean", "z_var", "z_std", "z_hist_n", "z_p50", "z_p95"]
    ZC.same_table(got, want, f"{chunks} chunks")
    assert got["zone"].dtype == np.int32 and got["points"].dtype == I64 and got["z_n"].dtype == U64 and got["z_p95"].dtype == F32
    assert len(got["zone"]) == 14 and (got["points"] > 0).all() and int(got["points"].sum()) > 1000 and (got["z_n"].astype(I64) < got["points"]).all()
    P.bits_equal(p.point_zonal_histogram(0, 0), counts[0], "point_zonal_histogram")
    p.finalize()                                                             # finalize neither needs nor changes it
    ZC.same_table(p.point_zonal(0), want, "after finalize")
    with pytest.raises(RuntimeError, match="no point_zonal entry 1"):
        p.point_zonal(1)
    with pytest.raises(RuntimeError, match="no histogram 1 in the entry"):
        p.point_zonal_histogram(0, 1)


def test_any_float32_channel_labels_and_the_free_function(plot_case):
    """The cloud's own channel as the label (`cls`: one row per class), and pcr.point_zonal on the same cloud."""
    import sample_grid_common as SG
    polys, c, labels, _, _ = plot_case
    want, counts = P.pipeline_model(c, c["cls"], 8)
    assert want["points"].tolist()[0] > 0 and want["points"].tolist()[2:4] == [0, 0] and len(want["zone"]) == 5
    p = P.plot_pipeline(pcr, "cpu", label="cls", max_zones=8)
    p.set_polygons("plot", polys.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c))
    ZC.same_table(p.point_zonal(0), want, "cls")
    e = P.entry(pcr)
    free = pcr.point_zonal(SG.dict_cloud(pcr, c), "cls", e.cell_stats, e.histograms, max_zones=8)
    ZC.same_table(free, want, "pcr.point_zonal")
    with pytest.raises(RuntimeError, match="a spec's filter needs a pipeline"):
        pcr.point_zonal(SG.dict_cloud(pcr, c), "cls", P.entry(pcr, stat_filt=P.STAT_FILT).cell_stats)
    with pytest.raises(RuntimeError, match="point_zonal label channel not found: plot"):
        pcr.point_zonal(SG.dict_cloud(pcr, c), "plot")
    only = pcr.point_zonal(SG.dict_cloud(pcr, c), "cls")
    assert list(only) == ["zone", "points"] and only["points"].tolist() == want["points"].tolist()


def test_a_label_above_max_zones_is_out_of_range(plot_case):
    import sample_grid_common as SG
    polys, c, labels, _, _ = plot_case
    p = P.plot_pipeline(pcr, "cpu", max_zones=5)
    p.set_polygons("plot", polys.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c))
    over = int((labels > 5).sum())
    with pytest.raises(RuntimeError, match=f"{over} points of 'plot' carry a zone above max_zones = 5"):
        p.point_zonal(0)
    with pytest.raises(RuntimeError, match="carry a zone above max_zones = 5"):
        p.point_zonal_histogram(0, 0)


def test_checkpoints_are_refused(plot_case, tmp_path):
    p = filtered_pipeline(plot_case[0])
    for call in (p.save_state, p.load_state):
        with pytest.raises(RuntimeError, match="checkpoints do not carry the point zonal tables"):
            call(str(tmp_path))
    import reduction_filters_common as RF
    import sample_grid_common as SG
    cfg = RF.make_config("cpu", [RF.S("Count", ch="z")], (), SG.PGRID, point_zonal=[P.entry(pcr, label="cls")])
    cfg.state_dir, cfg.resume = str(tmp_path), True
    assert pcr.Pipeline.create(cfg) is None
    assert "checkpoints do not carry the point zonal tables" in pcr.pipeline_create_error()


def test_create_refusals():
    import reduction_filters_common as RF
    import sample_grid_common as SG

    def refused(entries, mode="cpu", **kw):
        cfg = RF.make_config(mode, [RF.S("Count", ch="z")], (), SG.PGRID, point_zonal=entries)
        for k, v in kw.items():
            setattr(cfg, k, v)
        assert pcr.Pipeline.create(cfg) is None
        return pcr.pipeline_create_error()

    def with_(what, **fields):
        e = P.entry(pcr)
        spec = (e.cell_stats if what == "cell_stats" else e.histograms)[0]
        for k, v in fields.items():
            setattr(spec, k, v)
        setattr(e, what, [spec])
        return [e]

    ok = P.entry(pcr)
    assert refused([ok] * 5) == "pipeline: point_zonal: more than 4 entries"
    assert refused([pcr.PointZonalConfig("plot", ok.cell_stats * 5)]) == "pipeline: point_zonal[0]: more than 4 cell_stats specs"
    assert refused([ok, pcr.PointZonalConfig("plot", [], ok.histograms * 5)]) == "pipeline: point_zonal[1]: more than 4 histograms"
    assert refused([pcr.PointZonalConfig("")]) == "pipeline: point_zonal[0].label_channel is empty"
    assert refused([pcr.PointZonalConfig("plot", ok.cell_stats * 2)]) == "pipeline: point_zonal[0]: column 'z_mean' appears twice"
    e = P.entry(pcr)
    h = e.histograms[0]
    h.percentiles = [0.5, 0.501]
    e.histograms = [h]
    assert "point_zonal[0]: column 'z_p50' appears twice" in refused([e])
    for bad in (0, -4, 2 ** 24 + 1):
        assert refused([P.entry(pcr, max_zones=bad)]) == "pipeline: point_zonal[0].max_zones must be between 1 and 2^24"
    # the per-spec refusals of the per-cell stats and histograms
    assert refused(with_("cell_stats", value_channel="")) == "pipeline: point_zonal[0].cell_stats[0].value_channel is empty"
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):
        assert refused(with_("cell_stats", resolution=bad)) == "pipeline: point_zonal[0].cell_stats[0].resolution must be finite and positive"
    assert refused(with_("cell_stats", origin=float("inf"))) == "pipeline: point_zonal[0].cell_stats[0].origin must be finite"
    assert refused(with_("cell_stats", ddof=2)) == "pipeline: point_zonal[0].cell_stats[0].ddof must be 0 or 1"
    assert refused(with_("histograms", value_channel="")) == "pipeline: point_zonal[0].histograms[0].value_channel is empty"
    for bad in (0, 257):
        assert refused(with_("histograms", bins=bad)) == "pipeline: point_zonal[0].histograms[0].bins must be between 1 and 256"
    assert "histograms[0] needs finite bounds with lo < hi" in refused(with_("histograms", lo=64.0))
    assert "histograms[0] has more than 16 percentiles" in refused(with_("histograms", percentiles=[0.5] * 17))
    assert "histograms[0].percentiles must lie in [0, 1]" in refused(with_("histograms", percentiles=[1.5]))
    # its filters join the one plan and stay under its limits
    many = [P.entry(pcr, stat_filt=[("ret", "Equal", float(k))], hist_filt=[("ret", "Equal", float(k + 10))]) for k in range(4)]
    cfg = RF.make_config("cpu", [RF.S("Count", ch="z")], (), SG.PGRID, point_zonal=many)
    assert pcr.Pipeline.create(cfg) is not None, pcr.pipeline_create_error()    # eight distinct filters: the plan's limit
    assert "more than 8 distinct reduction filters" in refused(many, histograms=[_hist_with_filter()])
    for mode in ("cpu", "gpu"):                                               # a row-block shard, on either engine
        assert "point_zonal tables are not supported on a row-block shard" in refused([ok], mode, shard_row_begin=0, shard_row_end=16)


def _hist_with_filter():
    import reduction_filters_common as RF
    h = pcr.HistogramConfig("z", 0.0, 64.0, 8, [0.5])
    h.filter = RF.filter_spec([("ret", "Equal", 77.0)])
    return h


def test_an_empty_list_changes_nothing(plot_case):
    import reduction_filters_common as RF
    import sample_grid_common as SG
    p = pcr.Pipeline.create(RF.make_config("cpu", [RF.S("Count", ch="z")], (), SG.PGRID))
    p.ingest(SG.dict_cloud(pcr, plot_case[1]))
    with pytest.raises(RuntimeError, match="no point_zonal entry 0"):
        p.point_zonal(0)
    assert pcr.PipelineConfig().point_zonal == []


# ---- 4: agreement with the per-cell table -----------------------------------------------------------------------------------------
def test_equals_the_per_cell_table_when_every_point_has_its_cells_zone():
    """A label grid with the pipeline's own geometry, sampled Nearest: a point's label is its cell's, and all points lie inside
    the grid -- the group-by over points and the fold of the per-cell planes by the same grid are then the same sums."""
    import overviews_common as OC
    import reduction_filters_common as RF
    import sample_grid_common as SG
    g = SG.PGRID
    labels = ZC.plot_labels(g["W"], g["H"], plot=8)
    rng = np.random.default_rng(4)
    c = SG.one_point_per_cell(11)
    more = 4000
    c = dict(x=np.concatenate([c["x"], rng.uniform(0.01, 39.99, more)]), y=np.concatenate([c["y"], rng.uniform(0.01, 23.99, more)]),
             z=np.concatenate([c["z"], rng.uniform(-5.0, 70.0, more).astype(F32)]))
    c["z"][::37] = np.nan
    e = P.entry(pcr, label="plot_of_cell")
    cfg = RF.make_config("cpu", [RF.S("Count", ch="z")], (), g,
                         surface_channels=SG.channel_configs(pcr, [("plot_of_cell", "", SG.NEAREST)]),
                         cell_stats=list(e.cell_stats), histograms=list(e.histograms),
                         zonal=[pcr.ZonalConfig("plots", external=True, cell_stats=[0], histograms=[0])], point_zonal=[e])
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    SG.set_surfaces(pcr, p, {"plot_of_cell": SG.Surface(labels, g["min_x"], g["max_y"], g["cs"], -g["cs"])})
    p.ingest(SG.dict_cloud(pcr, c))
    p.finalize()
    p.set_zones("plots", OC.make_grid([labels]))
    per_cell, per_point = p.zonal(0), p.point_zonal(0)
    assert list(per_cell)[2:] == list(per_point)[2:] and len(per_point["zone"]) == len(per_cell["zone"]) == ZC.zone_max(labels)
    for k in list(per_cell)[2:] + ["zone"]:
        P.bits_equal(per_point[k], per_cell[k], f"column {k}")
    assert int(per_point["points"].sum()) > 4000 and (per_point["z_n"].astype(I64) <= per_point["points"]).all()
    P.bits_equal(p.point_zonal_histogram(0, 0), p.zonal_histogram(0, 0), "the counts")


def test_specs_whose_constants_round_give_both_tables_the_same_bits():
    """lo = 0.1, hi = 37.3, bins = 7 and resolution = 0.03: 1 / resolution, bins / (hi - lo) and (hi - lo) / bins all round, so
    the two tables agree only while one routine makes a spec's constants for both.  A few hundred points on a 16 x 16 grid, each
    labelled with its cell's zone."""
    import overviews_common as OC
    import reduction_filters_common as RF
    import sample_grid_common as SG
    g = dict(min_x=0.0, min_y=0.0, max_x=16.0, max_y=16.0, cs=1.0, W=16, H=16, tw=16, th=16)
    labels = ZC.plot_labels(16, 16, plot=4)
    rng = np.random.default_rng(9)
    n = 300
    c = dict(x=rng.uniform(0.01, 15.99, n), y=rng.uniform(0.01, 15.99, n), z=rng.uniform(-3.0, 41.0, n).astype(F32))
    c["z"][::29] = np.nan
    c["plot"] = labels[np.floor(16.0 - c["y"]).astype(int), np.floor(c["x"]).astype(int)]
    cs = pcr.CellStatsConfig("z", 0.7, 0.03, [pcr.CellStat.Mean], 1)
    h = pcr.HistogramConfig("z", 0.1, 37.3, 7, [0.1, 0.5, 0.9])
    cfg = RF.make_config("cpu", [RF.S("Count", ch="z")], (), g, cell_stats=[cs], histograms=[h],
                         zonal=[pcr.ZonalConfig("plots", external=True, cell_stats=[0], histograms=[0])],
                         point_zonal=[pcr.PointZonalConfig("plot", [cs], [h], 64)])
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    p.ingest(SG.dict_cloud(pcr, c))
    p.finalize()
    p.set_zones("plots", OC.make_grid([labels]))
    per_cell, per_point = p.zonal(0), p.point_zonal(0)
    assert list(per_cell)[2:] == list(per_point)[2:] == ["z_n", "z_mean", "z_var", "z_std", "z_hist_n", "z_p10", "z_p50", "z_p90"]
    assert len(per_point["zone"]) == len(per_cell["zone"]) == ZC.zone_max(labels) and int(per_point["z_n"].sum()) > 200
    for k in list(per_cell)[2:]:
        P.bits_equal(per_point[k], per_cell[k], f"column {k}")
    P.bits_equal(p.point_zonal_histogram(0, 0), p.zonal_histogram(0, 0), "the counts")


# ---- 5: why the feature exists ---------------------------------------------------------------------------------------------------
def test_a_plots_count_is_exact_where_the_cell_route_is_not():
    """One triangular plot on a 10 m grid, points on a 1 m lattice off every cell centre and edge: the `points` column is NumPy's
    count of points_in_polygons' channel; the per-cell route (the plot burnt into the grid, the cells' N folded by it) counts the
    points of the cells whose CENTRE the plot holds -- another number."""
    import reduction_filters_common as RF
    import sample_grid_common as SG
    g, polys, c = P.triangle_case()
    cloud = SG.dict_cloud(pcr, c)
    pcr.points_in_polygons(cloud, polys.to_pcr(), "plot")
    exact = int((np.asarray(cloud.channel_array_f32("plot")) == 1.0).sum())
    e = P.entry(pcr, hist=False)
    cfg = RF.make_config("cpu", [RF.S("Count", ch="z")], (), g, polygon_channels=[pcr.PolygonChannelConfig("plot")],
                         cell_stats=list(e.cell_stats), zonal=[pcr.ZonalConfig("plots", external=True, cell_stats=[0])], point_zonal=[e])
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    p.set_polygons("plot", polys.to_pcr())
    p.set_zones("plots", polys.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c))
    p.finalize()
    per_point, per_cell = p.point_zonal(0), p.zonal(0)
    assert per_point["points"].tolist() == [exact] and per_point["z_n"].tolist() == [exact]
    by_cells = int(per_cell["z_n"][0])
    assert by_cells == 100 * int(per_cell["cells"][0]) and by_cells != exact, (by_cells, exact)      # (3000 against 3003)


# ---- 6: sanitizers (the twins' loops alone, in a program of their own) ----------------------------------------------------------
def test_twin_loops_under_asan_ubsan(tmp_path):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "point_zonal_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=undefined,float-cast-overflow", "-fno-omit-frame-pointer",
                    "-I", os.path.join(root, "pointcloud-raster_amd", "csrc"), os.path.join(root, "tests", "native", "point_zonal_san.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "the twins' loops survived" in out.stdout
