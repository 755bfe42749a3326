"""Zonal tables on the host: the C-ABI's host twins (pcr_hip_zone_*_host) held BIT FOR BIT to the model of the contract in
tests/zonal_common.py -- label edge values, a zone with no cell, sums that carry past 2^32 and 2^63, n <= ddof, 1, 32 and 256
bins, a rank that lands on a bin of more than 2^32 points -- and the host engine's PipelineConfig.zonal: Pipeline.zonal against
the model applied to the pipeline's own planes, cube and tree_id band, the two-cone known answer, every refusal."""
import numpy as np
import pytest

import ground_filter_common as G
import histogram_common as H
import pcr
import trees_common as T
import zonal_common as Z
from conftest import load_cabi

F32, U32, I64, U64 = np.float32, np.uint32, np.int64, np.uint64
CPU = pcr.ExecutionMode.CPU


@pytest.fixture(scope="module")
def A():
    return load_cabi()


# ---- 1: the host twins against the model ---------------------------------------------------------------------------------------
def test_zone_of_a_label(A):
    cases = {float("nan"): 0, float("inf"): 0, -float("inf"): 0, 0.0: 0, -0.0: 0, -3.0: 0, 2.5: 0, 0.5: 0, 1.0: 1, 7.0: 7,
             float(2 ** 24): 2 ** 24, float(2 ** 24 + 1): 2 ** 24,           # (2^24 + 1 is no Float32: the band holds 2^24)
             float(2 ** 24 + 2): 0, float(2 ** 24 - 1): 2 ** 24 - 1, 1e30: 0, 1.0000001: 0}
    for v, want in cases.items():
        assert Z.zone_of(v) == want, v
        assert Z.run_zone_max(A, False, np.array([[v]], F32)) == want, v
    labels = np.array([[np.nan, 3.0, -1.0], [2.5, 9.0, np.inf]], F32)
    assert Z.run_zone_max(A, False, labels) == 9 == Z.zone_max(labels)
    assert Z.run_zone_max(A, False, labels, stride=8, offset=3) == 9


@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (3, 65), (33, 200)])
def test_folds_equal_the_model(A, shape):
    h, w = shape
    planes = Z.random_planes(h, w, 7)
    cube = Z.random_cube(5, h, w, 8)
    for name, (labels, zmax) in Z.label_patterns(h, w).items():
        for stride, offset in ((w, 0), (w + 5, 3)):
            what = f"{shape} {name} stride {stride} offset {offset}"
            want = Z.fold(labels, zmax, planes=planes, cube=cube)
            got = Z.run_fold_stats(A, False, labels, planes, zmax, stride=stride, offset=offset)
            for k in ("cells", "n", "s1", "s2"):
                Z.bits_equal(got[k], want[k], f"{what}: {k}")
            Z.bits_equal(Z.run_fold_hist(A, False, labels, cube, zmax, stride=stride, offset=offset, gap=offset), want["counts"], what)
        only = Z.run_fold_stats(A, False, labels, None, zmax)
        assert list(only) == ["cells"]
        Z.bits_equal(only["cells"], want["cells"], f"{shape} {name}: cells alone")
        none = Z.run_fold_stats(A, False, labels, planes, zmax, cells=False)
        assert "cells" not in none
        Z.bits_equal(none["n"], want["n"], f"{shape} {name}: no cells")


def test_a_zone_with_no_cell_and_labels_at_the_edges(A):
    labels = np.array([[1.0, 4.0, np.nan, np.inf, -np.inf, 0.0, -3.0, 2.5, -0.0, 4.0, float(2 ** 24), float(2 ** 24 + 2)]], F32)
    planes = Z.random_planes(1, 12, 1)
    want = Z.fold(labels, 4, planes=planes)
    assert want["cells"].tolist() == [1, 0, 0, 2]                          # zones 2 and 3 have no cell; 2^24 is above the Z passed in
    got = Z.run_fold_stats(A, False, labels, planes, 4)
    for k in want:
        Z.bits_equal(got[k], want[k], k)
    mean, var, std = Z.run_rows_stats(A, False, got["n"], got["s1"], got["s2"], 0.0, 0.01, 0)
    assert np.isnan(mean[1:3]).all() and np.isnan(std[1:3]).all()
    assert Z.run_zone_max(A, False, labels) == 2 ** 24


@pytest.mark.parametrize("ddof", [0, 1])
def test_sums_that_carry(A, ddof):
    labels, planes, zmax = Z.carry_planes()
    want = Z.fold(labels, zmax, planes=planes)
    assert int(want["n"][0]) > 2 ** 32 and int(want["cells"][0]) == 6
    s2_terms = [int(v) for v, z in zip(planes[2][0], labels[0]) if z == 1]
    assert sum(s2_terms[:3]) > 2 ** 63 and sum(s2_terms) > 2 ** 64         # carries past 2^63, then wraps
    run, signs = 0, set()
    for v, z in zip(planes[1][0], labels[0]):
        if z == 1:
            run += int(v)
            signs.add(run > 0)
    assert signs == {True, False}                                          # s1 changes sign on the way
    assert want["cells"].tolist() == [6, 1, 2, 0, 1] and want["n"].tolist()[1:] == [1, 0, 0, 7]
    got = Z.run_fold_stats(A, False, labels, planes, zmax)
    for k in want:
        Z.bits_equal(got[k], want[k], k)
    for origin, res in ((0.0, 0.01), (-2.0, 2.0 ** -6)):
        cols = Z.run_rows_stats(A, False, got["n"], got["s1"], got["s2"], origin, res, ddof)
        for name, g, m in zip(("mean", "var", "std"), cols, Z.rows_stats(want["n"], want["s1"], want["s2"], origin, res, ddof)):
            Z.bits_equal(g, m, f"ddof {ddof} res {res}: {name}")
        mean, var, std = cols
        assert not np.isnan(mean[0]) and not np.isnan(mean[1]) and np.isnan(mean[2]) and np.isnan(mean[3])
        assert np.isnan(var[1]) == (ddof == 1) and np.isnan(std[1]) == (ddof == 1)      # n = 1 <= ddof


def test_rows_of_preset_states(A):
    import cell_stats_common as K
    n, s1, s2 = (a.reshape(-1) for a in K.preset_states())
    n64 = n.astype(U64)
    n64[5] = (1 << 40) + 3                                                 # a count no cell can hold
    for ddof in (0, 1):
        got = Z.run_rows_stats(A, False, n64, s1, s2, 1.5, 0.125, ddof)
        for name, g, m in zip(("mean", "var", "std"), got, Z.rows_stats(n64, s1, s2, 1.5, 0.125, ddof)):
            Z.bits_equal(g, m, f"ddof {ddof}: {name}")
    # a zone of ONE cell is that cell: the rows are the per-cell bands
    bands = K.bands(n, s1, s2, 1.5, 0.125, 1)
    got = Z.run_rows_stats(A, False, n.astype(U64), s1, s2, 1.5, 0.125, 1)
    for p, g in zip((K.MEAN, K.VARIANCE, K.STDDEV), got):
        Z.bits_equal(g, bands[p].reshape(-1), f"product {p}")


@pytest.mark.parametrize("bins", [1, 32, 256])
def test_histogram_rows(A, bins):
    qs = [0.0, 0.25, 0.5, 0.95, 1.0]
    lo, w = Z.hist_consts(-3.0, 61.0, bins)
    h, wd = 3, 65
    labels, zmax = Z.label_patterns(h, wd)["invalid labels scattered in"]
    cube = Z.random_cube(bins, h, wd, bins)
    want = Z.fold(labels, zmax + 1, cube=cube)["counts"]                   # (the last zone has no cell)
    got = Z.run_fold_hist(A, False, labels, cube, zmax + 1)
    Z.bits_equal(got, want, "counts")
    hist_n, cols = Z.run_rows_percentiles(A, False, got, lo, w, qs)
    m_n, m_cols = Z.rows_percentiles(want, lo, w, qs)
    Z.bits_equal(hist_n, m_n, "hist_n")
    for q, g, m in zip(qs, cols, m_cols):
        Z.bits_equal(g, m, f"q {q}")
    assert hist_n[-1] == 0 and np.isnan(cols[2][-1]) and not np.isnan(cols[2][0])
    only_n, none = Z.run_rows_percentiles(A, False, got, lo, w, [])
    Z.bits_equal(only_n, m_n, "hist_n alone")
    # a zone of one cell is that cell: the rows are the percentile bands
    one = np.arange(1, wd + 1, dtype=F32)[None, :]
    c1 = Z.random_cube(bins, 1, wd, 3)
    _, cols = Z.run_rows_percentiles(A, False, Z.run_fold_hist(A, False, one, c1, wd), lo, w, qs)
    for g, band in zip(cols, H.percentiles(c1, -3.0, 61.0, bins, qs)):
        Z.bits_equal(g, band.reshape(-1), "against the per-cell bands")


@pytest.mark.parametrize("bins", [1, 32, 256])
def test_a_rank_in_a_bin_of_more_than_2_32_points(A, bins):
    labels, cube, zmax = Z.carry_cube(bins)
    want = Z.fold(labels, zmax, cube=cube)["counts"]
    assert int(want[0, bins - 1]) > 2 ** 32
    got = Z.run_fold_hist(A, False, labels, cube, zmax)
    Z.bits_equal(got, want, "counts")
    qs = [0.0, 0.5, 0.95, 1.0]
    lo, w = Z.hist_consts(0.0, 64.0, bins)
    hist_n, cols = Z.run_rows_percentiles(A, False, got, lo, w, qs)
    m_n, m_cols = Z.rows_percentiles(want, lo, w, qs)
    Z.bits_equal(hist_n, m_n, "hist_n")
    assert int(hist_n[0]) > 2 ** 32
    for q, g, m in zip(qs, cols, m_cols):
        Z.bits_equal(g, m, f"q {q}")
    assert cols[3][0] > lo + w * (bins - 1)                                # q = 1 lands in the last bin, the one of 2^34 - 4 points


def test_argument_errors(A):
    L = A.lib()
    import ctypes as C
    lab = np.ones((4, 8), F32)
    n, s1, s2 = np.zeros((4, 8), U32), np.zeros((4, 8), I64), np.zeros((4, 8), U64)
    t = [np.zeros(8, U64) for _ in range(4)]
    t[2] = t[2].view(I64)
    cube = np.zeros((2, 4, 8), U32)
    zc = np.zeros(16, U64)
    prm, bad_prm = A.ZoneFoldParams(1), A.ZoneFoldParams(2)
    p = lambda a: a.ctypes.data
    P = C.byref(prm)

    def stats(lab_p=p(lab), w=8, h=4, ls=8, n_p=p(n), s1_p=p(s1), s2_p=p(s2), ps=8, zmax=8, prm_p=P, c=p(t[0]), a=p(t[1]), b=p(t[2]), d=p(t[3])):
        return L.pcr_hip_zone_fold_stats_host(lab_p, w, h, ls, n_p, s1_p, s2_p, ps, zmax, prm_p, c, a, b, d)

    def hist(lab_p=p(lab), w=8, h=4, ls=8, c_p=p(cube), bins=2, cs=8, bs=32, zmax=8, prm_p=P, z_p=p(zc)):
        return L.pcr_hip_zone_fold_hist_host(lab_p, w, h, ls, c_p, bins, cs, bs, zmax, prm_p, z_p)

    assert stats() == 0 and hist() == 0
    for kw, msg in ((dict(lab_p=None), "null argument"), (dict(prm_p=None), "null argument"), (dict(s1_p=None), "null argument"),
                    (dict(c=None, n_p=None, s1_p=None, s2_p=None, a=None, b=None, d=None), "null argument"),
                    (dict(w=0), "width and height must be positive"), (dict(h=-1), "width and height must be positive"),
                    (dict(ls=7), "zone_stride smaller than width"), (dict(ps=7), "plane_stride smaller than width"),
                    (dict(zmax=0), "Z must be between 1 and 2^24"), (dict(zmax=2 ** 24 + 1), "Z must be between 1 and 2^24"),
                    (dict(w=2 ** 16, h=2 ** 15, ls=2 ** 16, ps=2 ** 16), "more than 2^31 - 1 cells"),
                    (dict(prm_p=C.byref(bad_prm)), "combine must be 0 or 1"),
                    (dict(c=p(lab)), "a table overlaps an input"), (dict(a=p(s2) + 8), "a table overlaps an input"),
                    (dict(d=p(t[0])), "two tables overlap")):
        assert stats(**kw) != 0, kw
        assert msg in L.pcr_hip_last_error().decode(), (kw, L.pcr_hip_last_error())
    for kw, msg in ((dict(c_p=None), "null argument"), (dict(z_p=None), "null argument"), (dict(bins=0), "bins must be between 1 and 256"),
                    (dict(bins=257), "bins must be between 1 and 256"), (dict(cs=7), "count_stride smaller than width"),
                    (dict(bs=31), "bin_stride smaller than a plane"), (dict(zmax=0), "Z must be between 1 and 2^24"),
                    (dict(ls=7), "zone_stride smaller than width"), (dict(z_p=p(cube) + 64), "the table overlaps an input"),
                    (dict(z_p=p(lab)), "the table overlaps an input")):
        assert hist(**kw) != 0, kw
        assert msg in L.pcr_hip_last_error().decode(), (kw, L.pcr_hip_last_error())
    out = C.c_uint32(0)
    assert L.pcr_hip_zone_max_host(None, 8, 4, 8, C.byref(out)) != 0 and "null argument" in L.pcr_hip_last_error().decode()
    assert L.pcr_hip_zone_max_host(p(lab), 8, 4, 7, C.byref(out)) != 0 and "zone_stride smaller" in L.pcr_hip_last_error().decode()
    cols = [np.zeros(8, F32) for _ in range(3)]
    rows = lambda zmax=8, ddof=0, res=0.01, m=p(cols[0]): L.pcr_hip_zone_rows_stats_host(p(t[1]), p(t[2]), p(t[3]), zmax, 0.0, res, ddof, m,
                                                                                       p(cols[1]), p(cols[2]))
    assert rows() == 0
    for kw, msg in ((dict(zmax=0), "Z must be"), (dict(ddof=2), "ddof must be 0 or 1"), (dict(res=0.0), "resolution positive"),
                    (dict(m=p(t[1])), "a column overlaps an input")):
        assert rows(**kw) != 0 and msg in L.pcr_hip_last_error().decode(), kw
    q = np.array([0.5, 1.5], F32)
    ptrs = (C.c_void_p * 2)(p(cols[0]), p(cols[1]))
    pct = lambda bins=2, nq=1, lo=0.0, w=1.0: L.pcr_hip_zone_rows_percentiles_host(p(zc), bins, 8, lo, w, nq, p(q), p(t[0]), ptrs)
    assert pct() == 0
    for kw, msg in ((dict(bins=0), "bins must be"), (dict(nq=17), "between 0 and 16 percentiles"), (dict(nq=2), "must lie in [0, 1]"),
                    (dict(w=0.0), "w positive"), (dict(lo=float("nan")), "must be finite")):
        assert pct(**kw) != 0 and msg in L.pcr_hip_last_error().decode(), kw


# ---- 2: the host engine's PipelineConfig.zonal ---------------------------------------------------------------------------------
WP, HP = 130, 70


def test_pipeline_equals_the_model():
    pipe = Z.create(pcr, Z.pipeline_cfg(pcr, WP, HP, CPU), "host")
    with pytest.raises(RuntimeError, match="no zonal entry 0"):
        pipe.zonal(0)                                                     # before the first finalize
    c1, c2 = Z.canopy_points(pcr, WP, HP, 1), Z.canopy_points(pcr, WP, HP, 2)
    for k, c in enumerate((c1, c2)):
        pipe.ingest(c)
        with pytest.raises(RuntimeError, match="no zonal entry 0"):
            pipe.zonal(0)                                                 # after a further ingest
        with pytest.raises(RuntimeError, match="no zonal entry 0"):
            pipe.zonal_histogram(0, 0)
        pipe.finalize()
        want, counts = Z.pipeline_model(pcr, pipe)
        got = pipe.zonal(0)
        Z.same_table(got, want, f"finalize {k + 1}")
        Z.bits_equal(pipe.zonal_histogram(0, 0), counts[0], f"finalize {k + 1}: zonal_histogram")
        trees = pipe.trees(0)
        assert len(got["zone"]) == len(trees["row"]) >= 50
        assert got["cells"].tolist() == trees["crown_cells"].tolist()
        assert got["cells"].dtype == np.int64 and got["zone"].dtype == np.int32 and got["value_n"].dtype == np.uint64
        assert got["value_p95"].dtype == F32 and (got["value_n"] >= got["cells"].astype(U64)).all()
        assert not np.isnan(got["value_std"]).all()
    with pytest.raises(RuntimeError, match="no zonal entry 1"):
        pipe.zonal(1)
    with pytest.raises(RuntimeError, match="no histogram 1 in the entry"):
        pipe.zonal_histogram(0, 1)


def test_a_cloud_the_pipeline_filter_empties_leaves_the_table_valid():
    """An ingest that PipelineConfig::filter keeps no point of changes no state: zonal(i) answers as before, as on the HIP
    engine (pipeline.h, Pipeline::zonal).  The host engine used to refuse it; the operation-sequence fuzz's model found the two
    engines apart."""
    cfg = Z.pipeline_cfg(pcr, WP, HP, CPU)
    cfg.filter.add("value", pcr.CompareOp.GreaterEqual, -1.0e30)
    pipe = Z.create(pcr, cfg, "host")
    pipe.ingest(Z.canopy_points(pcr, WP, HP, 1))
    pipe.finalize()
    before = pipe.zonal(0)
    pipe.ingest(Z._cloud(pcr, np.array([3.5, 20.5]), np.array([4.5, 30.5]), np.array([-1.0e31, -2.0e31], F32)))     # all filtered out
    Z.same_table(pipe.zonal(0), before, "after a cloud the filter empties")
    assert pipe.stats().points_processed == len(Z.CLOUDS[(WP, HP, 1)][0])
    pipe.ingest(Z._cloud(pcr, np.array([3.5]), np.array([4.5]), np.array([1.0], F32)))                             # one point that counts
    with pytest.raises(RuntimeError, match="no zonal entry 0"):
        pipe.zonal(0)


def test_two_cones_known_answer():
    z = Z.cones()
    pipe = Z.create(pcr, Z.pipeline_cfg(pcr, 40, 32, CPU), "host")
    pipe.ingest(Z.cloud_of_band(pcr, z))
    pipe.finalize()
    got, trees = pipe.zonal(0), pipe.trees(0)
    assert got["cells"].tolist() == trees["crown_cells"].tolist() == [97, 37]
    assert got["zone"].tolist() == [1, 2] and got["value_n"].tolist() == [97, 37] and got["value_hist_n"].tolist() == [97, 37]


def test_external_zones_and_own_percentiles():
    cfg = Z.pipeline_cfg(pcr, WP, HP, CPU)
    cfg.zonal = [pcr.ZonalConfig("plots", external=True, cell_stats=[0], histograms=[0], percentiles=[0.1, 0.9]),
                 pcr.ZonalConfig("value_1_tree_id"),                                       # cells alone
                 pcr.ZonalConfig("value_5", histograms=[0], max_zones=3)]                  # any band: the Count band
    assert cfg.zonal[0].percentiles == pytest.approx([0.1, 0.9]) and cfg.zonal[1].percentiles is None
    pipe = Z.create(pcr, cfg, "host")
    pipe.ingest(Z.canopy_points(pcr, WP, HP, 1))
    pipe.finalize()
    with pytest.raises(RuntimeError, match="the label grid 'plots' was not set"):
        pipe.zonal(0)
    plots = Z.plot_labels(WP, HP)
    for bad in (T.make_grid([plots[:, :-1]]), T.make_grid([plots[:-1]])):
        with pytest.raises(RuntimeError, match="set_zones: the grid is"):
            pipe.set_zones("plots", bad)
    with pytest.raises(RuntimeError, match="'stands' names no external label grid"):
        pipe.set_zones("stands", T.make_grid([plots]))
    with pytest.raises(RuntimeError, match="band index outside the grid"):
        pipe.set_zones("plots", T.make_grid([plots]), 1)
    pipe.set_zones("plots", T.make_grid([np.zeros_like(plots), plots]), 1)
    want, counts = Z.pipeline_model(pcr, pipe, labels=plots, qs=[0.1, 0.9])
    got = pipe.zonal(0)
    assert list(got) == ["zone", "cells", "value_n", "value_mean", "value_var", "value_std", "value_hist_n", "value_p10", "value_p90"]
    Z.same_table(got, want, "plots")
    cells = pipe.zonal(1)
    assert list(cells) == ["zone", "cells"] and cells["cells"].tolist() == pipe.trees(0)["crown_cells"].tolist()
    with pytest.raises(RuntimeError, match="is above max_zones = 3"):      # the Count band holds cells of more than 3 points
        pipe.zonal(2)


def test_create_refusals():
    def refused(zonal, **kw):
        cfg = Z.pipeline_cfg(pcr, WP, HP, kw.pop("mode", CPU))
        cfg.zonal = zonal
        for k, v in kw.items():
            setattr(cfg, k, v)
        assert pcr.Pipeline.create(cfg) is None
        return pcr.pipeline_create_error()
    ok = pcr.ZonalConfig("value_1_tree_id", cell_stats=[0], histograms=[0])
    assert refused([pcr.ZonalConfig(f"g{k}", external=True) for k in range(5)]) == "pipeline: zonal: more than 4 entries"
    assert "zonal[1].zones 'plots' names no band of the result" in refused([ok, pcr.ZonalConfig("plots")])
    assert refused([pcr.ZonalConfig("")]) == "pipeline: zonal[0].zones is empty"
    assert refused([pcr.ZonalConfig("plots", external=True, cell_stats=[1])]) == "pipeline: zonal[0].cell_stats: no cell_stats entry 1"
    assert refused([pcr.ZonalConfig("plots", external=True, cell_stats=[-1])]) == "pipeline: zonal[0].cell_stats: no cell_stats entry -1"
    assert refused([ok, pcr.ZonalConfig("plots", external=True, histograms=[0, 1])]) == "pipeline: zonal[1].histograms: no histogram 1"
    assert "zonal[0].percentiles: more than 16" in refused([pcr.ZonalConfig("value_5", histograms=[0], percentiles=[0.5] * 17)])
    for bad in (-0.1, 1.5, float("nan")):
        assert "zonal[0].percentiles: a percentile must lie in [0, 1]" in refused([pcr.ZonalConfig("value_5", histograms=[0], percentiles=[bad])])
    assert refused([pcr.ZonalConfig("value_5", cell_stats=[0, 0])]) == "pipeline: zonal[0]: column 'value_mean' appears twice"
    assert "column 'value_p50' appears twice" in refused([pcr.ZonalConfig("value_5", histograms=[0], percentiles=[0.5, 0.501])])
    for bad in (0, -4, 2 ** 24 + 1):
        assert refused([pcr.ZonalConfig("value_5", max_zones=bad)]) == "pipeline: zonal[0].max_zones must be between 1 and 2^24"
    for mode in (CPU, pcr.ExecutionMode.GPU):                                               # a row-block shard, on either engine
        cfg = G.pipeline_cfg(WP, HP, mode, ground=False)
        cfg.zonal = [pcr.ZonalConfig("plots", external=True)]
        cfg.shard_row_begin, cfg.shard_row_end = 16, 32
        assert pcr.Pipeline.create(cfg) is None
        assert "zonal tables need the whole grid" in pcr.pipeline_create_error()


def test_an_empty_list_changes_nothing():
    cfg = Z.pipeline_cfg(pcr, WP, HP, CPU)
    cfg.zonal = []
    pipe = Z.create(pcr, cfg, "host")
    pipe.ingest(Z.canopy_points(pcr, WP, HP, 1))
    pipe.finalize()
    with pytest.raises(RuntimeError, match="no zonal entry 0"):
        pipe.zonal(0)
    with pytest.raises(RuntimeError, match="names no external label grid"):
        pipe.set_zones("plots", T.make_grid([Z.plot_labels(WP, HP)]))
