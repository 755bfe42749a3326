"""Individual trees on the CPU: the host twin (csrc/trees.hpp) against the brute-force model of tests/trees_common.py bit for
bit, the known answers of the contract, every refusal, and the host-engine pipeline.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ground_filter_common as G
import overviews_common as M
import pcr
import trees_common as T
from conftest import load_cabi

F32 = np.float32
CPU = pcr.ExecutionMode.CPU
INF = float("inf")


@pytest.fixture(scope="module")
def A():
    return load_cabi()


# ---- 1: the host twin against the model ------------------------------------------------------------------------------------------
FIELDS = {}


def field(w, h, seed=1):
    """(band, model result) of a generated canopy, made once."""
    if (w, h, seed) not in FIELDS:
        z = T.canopy(w, h, seed)
        FIELDS[(w, h, seed)] = (z, T.model(z))
    return FIELDS[(w, h, seed)]


@pytest.mark.parametrize("w,h", [(1, 1), (7, 1), (1, 7), (63, 31), (64, 32), (65, 33), (130, 70)])
def test_host_twin_matches_the_model(A, w, h):
    z, m = field(w, h)
    if (w, h) == (130, 70):
        T.exercises_the_rules(z, m)
    T.same_result(T.host(z), m, "binding")
    for stride in (w, w + 5):
        T.same_result(T.host_cabi(A, z, stride), m, f"C-ABI stride {stride}")


@pytest.mark.parametrize("seed", [2, 3])
def test_host_twin_matches_the_model_with_other_parameters(A, seed):
    z, m0 = field(130, 70, seed)
    T.exercises_the_rules(z, m0)
    for kw in (dict(max_radius_cells=1), dict(max_radius_cells=32, window_base=20.0, window_slope=1.5),
               dict(window_base=0.0, window_slope=0.0), dict(min_height=5.0, min_crown_height=1.0, crown_ratio=0.8, max_crown_radius=3.0),
               dict(crown_ratio=0.0, max_crown_radius=INF, min_crown_height=-5.0)):
        m = T.model(z, **kw)
        T.same_result(T.host(z, T.spec(**kw)), m, str(kw))
        T.same_result(T.host_cabi(A, z, 133, **kw), m, str(kw))
    for cs in ((0.5, -0.5), (2.0, -1.0), (-1.0, 3.0)):
        m = T.model(z, *cs)
        T.same_result(T.host(z, None, *cs), m, str(cs))
        T.same_result(T.host_cabi(A, z, None, *cs), m, str(cs))


def test_height_band_may_be_left_out(A):
    z, m = field(65, 33)
    got = T.host_cabi(A, z, 70, want_height=False)
    T.bits_equal(got["id"], m["id"])


def test_special_values(A):
    z = np.zeros((9, 11), F32)
    z[4, 5], z[4, 6] = -0.0, 0.0                          # equal: the lower idx wins
    z[2, 2] = np.inf
    z[6, 8] = np.array([0x7FA00001], np.uint32).view(F32)[0]         # a signalling NaN with a payload
    z[1, 7] = 1e-41                                       # a denormal is a value
    for kw in (dict(min_height=-1.0, min_crown_height=-1.0), dict(min_height=0.0, min_crown_height=0.0, max_radius_cells=2)):
        m = T.model(z, **kw)
        T.same_result(T.host(z, T.spec(**kw)), m)
        T.same_result(T.host_cabi(A, z, 16, **kw), m)
        assert np.isnan(m["id"][2, 2]) and np.isnan(m["id"][6, 8])


# ---- 2: known answers ------------------------------------------------------------------------------------------------------------
def cones():
    rr, cc = np.mgrid[0:32, 0:40]
    return np.maximum(np.maximum(0.0, 20.0 - 2.0 * np.hypot(rr - 10, cc - 10)), np.maximum(0.0, 12.0 - 2.0 * np.hypot(rr - 10, cc - 24))).astype(F32)


def test_two_cones():
    t = T.host(cones())
    assert (t["table"]["row"].tolist(), t["table"]["col"].tolist()) == ([10, 10], [10, 24])
    assert t["table"]["crown_cells"].tolist() == [97, 37]
    assert t["table"]["height"].tolist() == [20.0, 12.0]
    assert t["table"]["x"].tolist() == [10.5, 24.5] and t["table"]["y"].tolist() == [-10.5, -10.5]
    assert (t["id"] == 1).sum() == 97 and (t["id"] == 2).sum() == 37
    assert set(np.unique(t["height"][~np.isnan(t["height"])])) == {12.0, 20.0}
    T.same_result(t, T.model(cones()))


def test_plateau_is_one_tree():
    z = np.zeros((12, 12), F32)
    z[3:8, 4:9] = 10.0
    t = T.host(z)
    assert (t["table"]["row"].tolist(), t["table"]["col"].tolist(), t["table"]["crown_cells"].tolist()) == ([3], [4], [25])
    assert (t["id"][3:8, 4:9] == 1).all() and np.isnan(t["id"]).sum() == 144 - 25


def test_ramp_is_one_long_chain():
    z = (5.0 + 0.01 * np.arange(3000)).astype(F32)[None, :]
    kw = dict(crown_ratio=0.0, max_crown_radius=INF)
    m = T.model(z, **kw)
    assert m["chain"] == 2999
    t = T.host(z, T.spec(**kw))
    assert (t["table"]["row"].tolist(), t["table"]["col"].tolist(), t["table"]["crown_cells"].tolist()) == ([0], [2999], [3000])
    assert (t["id"] == 1).all()
    T.same_result(t, m)
    T.same_result(T.host(z.T.copy(), T.spec(**kw)), T.model(z.T.copy(), **kw), "a column")


def test_window_grows_with_height():
    def spikes(a, b):
        z = np.zeros((21, 27), F32)
        z[10, 10], z[10, 16] = a, b
        return z
    sp = T.spec(window_slope=0.5)
    tall, low = T.host(spikes(28.0, 30.0), sp), T.host(spikes(8.0, 10.0), sp)
    assert (tall["table"]["col"].tolist(), low["table"]["col"].tolist()) == ([16], [10, 16])
    T.same_result(tall, T.model(spikes(28.0, 30.0), window_slope=0.5))
    T.same_result(low, T.model(spikes(8.0, 10.0), window_slope=0.5))


def minor_peak():
    """A cone of 20 at (10, 10) with a bump of 11 at (10, 16), where the cone is 8: a local maximum six cells from the top."""
    rr, cc = np.mgrid[0:21, 0:25]
    z = np.maximum(0.0, 20.0 - 2.0 * np.hypot(rr - 10, cc - 10))
    z[10, 16] = 11.0
    return z.astype(F32)


def test_suppressed_peak_joins_its_neighbour_by_step_3():
    z = minor_peak()
    kw = dict(window_base=13.0, window_slope=0.0)          # R = 6 everywhere: (10, 10) is in the disc of (10, 16)
    m = T.model(z, **kw)
    assert (10, 16) in m["step3"] and len(m["table"]["row"]) == 1
    t = T.host(z, T.spec(**kw))
    T.same_result(t, m)
    assert t["id"][10, 16] == 1 and t["height"][10, 16] == 20.0
    near = T.host(z, T.spec(max_crown_radius=5.0, **kw))  # the root is 6 cells away
    T.same_result(near, T.model(z, max_crown_radius=5.0, **kw))
    assert np.isnan(near["id"][10, 16]) and near["id"][10, 12] == 1
    assert near["table"]["crown_cells"][0] < t["table"]["crown_cells"][0]


def test_negative_tops_keep_their_own_cell():
    z = np.full((9, 9), -10.0, F32)
    z[4, 4] = -3.0
    kw = dict(min_height=-5.0, min_crown_height=-20.0)
    t = T.host(z, T.spec(**kw))
    T.same_result(t, T.model(z, **kw))
    assert t["table"]["row"].tolist() == [4] and t["id"][4, 4] == 1
    # -10 >= 0.45 * -3 is false: the neighbours carry no label, the top's own cell still does
    assert t["table"]["crown_cells"].tolist() == [1] and np.isnan(t["id"]).sum() == 80


def test_crown_cells_sum_and_id_order():
    z, m = field(130, 70)
    t = T.host(z)
    assert int(t["table"]["crown_cells"].sum()) == int((~np.isnan(t["id"])).sum()) == m["labelled"]
    idx = t["table"]["row"].astype(np.int64) * 130 + t["table"]["col"]
    assert (np.diff(idx) > 0).all()
    for k in (0, len(idx) // 2, len(idx) - 1):
        assert t["id"][t["table"]["row"][k], t["table"]["col"][k]] == k + 1
        assert (t["id"] == k + 1).sum() == t["table"]["crown_cells"][k]


def test_id_clamp():
    from pcr import _pcr
    assert _pcr._tree_id_value(1) == 1.0 and _pcr._tree_id_value(2 ** 24) == 16777216.0
    for i in (2 ** 24 + 1, 2 ** 24 + 2, 2 ** 31 - 1):
        v = np.array([_pcr._tree_id_value(i)], F32)
        assert v.view(np.uint32)[0] == T.NAN_BITS


# ---- 3: refusals -----------------------------------------------------------------------------------------------------------------
BAD_SPECS = [(dict(min_height=float("nan")), "min_height must be finite"),
             (dict(window_base=-1.0), "window_base must be finite and not negative"),
             (dict(window_base=INF), "window_base must be finite and not negative"),
             (dict(window_slope=-0.1), "window_slope must be finite and not negative"),
             (dict(window_slope=float("nan")), "window_slope must be finite and not negative"),
             (dict(max_radius_cells=0), "max_radius_cells must be between 1 and 32"),
             (dict(max_radius_cells=33), "max_radius_cells must be between 1 and 32"),
             (dict(min_crown_height=INF), "min_crown_height must be finite"),
             (dict(crown_ratio=1.5), "crown_ratio must be between 0 and 1"),
             (dict(crown_ratio=-0.1), "crown_ratio must be between 0 and 1"),
             (dict(crown_ratio=float("nan")), "crown_ratio must be between 0 and 1"),
             (dict(max_crown_radius=0.0), "max_crown_radius must be positive"),
             (dict(max_crown_radius=float("nan")), "max_crown_radius must be positive")]


def test_segment_trees_on_a_host_grid_and_its_errors():
    z, m = field(65, 33)
    g, table = pcr.segment_trees(T.make_grid([z, z + 1]), 0)
    assert [g.band_desc(b).name for b in range(2)] == ["tree_id", "tree_height"]
    T.same_result(dict(id=T.grid_bands(g)[0], height=T.grid_bands(g)[1], table=table), m)
    g, table = pcr.segment_trees(T.make_grid([z]), spec=T.spec(min_height=4.0), cell_size_x=2.0, cell_size_y=-2.0)
    T.same_result(dict(id=T.grid_bands(g)[0], height=T.grid_bands(g)[1], table=table), T.model(z, 2.0, -2.0, min_height=4.0))
    grid = T.make_grid([z])
    for kw, msg in BAD_SPECS:
        with pytest.raises(RuntimeError, match="segment_trees: " + msg):
            pcr.segment_trees(grid, 0, T.spec(**kw))
    for args, msg in (((grid, 1), "band index outside the grid"), ((grid, -1), "band index outside the grid"),
                      ((grid, 0, None, 0.0, -1.0), "cell sizes must be finite and not zero"),
                      ((grid, 0, None, 1.0, float("nan")), "cell sizes must be finite and not zero")):
        with pytest.raises(RuntimeError, match=msg):
            pcr.segment_trees(*args)
    d = pcr.BandDesc()
    d.name, d.dtype = "ids", pcr.DataType.Int32
    with pytest.raises(RuntimeError, match="segment_trees needs a Float32 band"):
        pcr.segment_trees(pcr.Grid.create(8, 8, [d]), 0)


def test_table_centres_follow_the_geometry():
    z = cones()
    g = T.make_grid([z])
    gc = pcr.GridConfig()
    gc.bounds = pcr.BBox(500000.0, 4100000.0, 500000.0 + 40 * 0.5, 4100000.0 + 32 * 0.5)
    gc.cell_size_x, gc.cell_size_y = 0.5, -0.5
    gc.compute_dimensions()
    g.set_geometry(gc)
    _, table = pcr.segment_trees(g, 0, None, 0.5, -0.5)
    m = T.model(z, 0.5, -0.5)
    assert table["row"].tolist() == m["table"]["row"].tolist()
    assert table["x"].tolist() == [500000.0 + (c + 0.5) * 0.5 for c in table["col"]]
    assert table["y"].tolist() == [4100000.0 + 16.0 - (r + 0.5) * 0.5 for r in table["row"]]


def test_cabi_argument_errors_need_no_gpu(A):
    L = A.lib()
    w, h = 16, 8
    src, ids, hts = (np.zeros(1024, F32) for _ in range(3))         # (each larger than the work area, which may be put on it)
    work = np.zeros(4096, np.uint8)
    n = C.c_size_t(0)
    assert L.pcr_hip_trees_work_bytes(w, h, C.byref(n)) == 0 and n.value >= 12 * w * h
    assert L.pcr_hip_trees_work_bytes(0, h, C.byref(n)) == 1 and b"width and height must be positive" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_work_bytes(w, h, None) == 1 and b"null argument" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_work_bytes(65536, 65536, C.byref(n)) == 1 and b"more than 2^31 - 1 cells" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_work_bytes(w, h, C.byref(n)) == 0
    p = T.params(A)

    def dev(msg, src_p=src.ctypes.data, w_=w, h_=h, ss=w, p_=p, id_p=ids.ctypes.data, si=w, h_p=hts.ctypes.data, sh=w,
            work_p=work.ctypes.data, wb=None):
        rc = L.pcr_hip_trees(src_p, w_, h_, ss, C.byref(p_) if p_ is not None else None, id_p, si, h_p, sh, work_p,
                             n.value if wb is None else wb, None)
        assert rc == 1, msg
        assert msg.encode() in L.pcr_hip_last_error(), L.pcr_hip_last_error()

    def twin(msg, src_p=src.ctypes.data, w_=w, h_=h, ss=w, p_=p, id_p=ids.ctypes.data, si=w, h_p=hts.ctypes.data, sh=w, cap=0):
        rc = L.pcr_hip_trees_host(src_p, w_, h_, ss, C.byref(p_) if p_ is not None else None, id_p, si, h_p, sh, None, cap, None, None,
                                  None, None)
        assert rc == 1, msg
        assert msg.encode() in L.pcr_hip_last_error(), L.pcr_hip_last_error()

    for f in (dev, twin):
        f("null argument", src_p=None)
        f("null argument", id_p=None)
        f("null argument", p_=None)
        f("width and height must be positive", w_=0)
        f("width and height must be positive", h_=-3)
        f("src_stride smaller than width", ss=w - 1)
        f("id_stride smaller than width", si=w - 1)
        f("height_stride smaller than width", sh=w - 1)
        f("id_dst overlaps src", id_p=src.ctypes.data + 4 * w)
        f("height_dst overlaps src", h_p=src.ctypes.data)
        f("height_dst overlaps id_dst", h_p=ids.ctypes.data + 4)
        for kw, msg in BAD_SPECS:
            f(msg, p_=T.params(A, **kw))
        f("0.5 / cell is not finite", p_=T.params(A, 0.0, 0.0))
        f("0.5 / cell is not finite", p_=T.params(A, float("nan"), -1.0))
    dev("null argument", work_p=None)
    dev("work_bytes too small", wb=n.value - 1)
    dev("the workspace overlaps src", work_p=src.ctypes.data)
    dev("the workspace overlaps id_dst", work_p=ids.ctypes.data)
    dev("the workspace overlaps height_dst", work_p=hts.ctypes.data)
    big = C.c_size_t(0)
    assert L.pcr_hip_trees_work_bytes(1, 32 * 65535 + 1, C.byref(big)) == 0
    # (refused before anything is read: the addresses only have to lie apart)
    dev("more than 65535 tile rows", w_=1, h_=32 * 65535 + 1, ss=1, si=1, sh=1, wb=big.value, src_p=1 << 40, id_p=2 << 40,
        h_p=3 << 40, work_p=4 << 40)
    twin("capacity must not be negative", cap=-1)
    k, r = C.c_int64(0), C.c_int(0)
    assert L.pcr_hip_trees_count(None, n.value, C.byref(k), C.byref(r), None) == 1 and b"null argument" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_count(work.ctypes.data, 8, C.byref(k), None, None) == 1 and b"work_bytes too small" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_table(None, w, h, w, work.ctypes.data, n.value, 1, None, None, None, None, None) == 1
    assert b"null argument" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_table(src.ctypes.data, w, h, w - 1, work.ctypes.data, n.value, 1, None, None, None, None, None) == 1
    assert b"src_stride smaller than width" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_table(src.ctypes.data, w, h, w, work.ctypes.data, 16, 1, None, None, None, None, None) == 1
    assert b"work_bytes too small" in L.pcr_hip_last_error()
    assert L.pcr_hip_trees_table(src.ctypes.data, w, h, w, work.ctypes.data, n.value, -1, None, None, None, None, None) == 1
    assert b"n must not be negative" in L.pcr_hip_last_error()


# ---- 4: the host-engine pipeline -------------------------------------------------------------------------------------------------
W, H, NPTS, RADIUS = 64, 48, 6000, 2


def run_pipeline(cfg, clouds):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "host"
    out = []
    for c in clouds:
        pipe.ingest(c)
        pipe.finalize()
        res = pipe.result()
        tables = [pipe.trees(i) for i in range(len(cfg.trees))]
        out.append(([res.band_desc(b).name for b in range(res.num_bands())], G.grid_bands(res), tables))
    return out


@pytest.fixture(scope="module")
def clouds():
    return G.cloud(W, H, NPTS, seed=81), G.cloud(W, H, NPTS // 4, seed=82)


def test_trees_are_off_by_default(clouds):
    cfg = pcr.PipelineConfig()
    assert list(cfg.trees) == []
    t = pcr.TreeBandConfig()
    assert (t.source_band, t.id_band_name, t.height_band_name) == ("", "", "")
    assert {k: getattr(t, k) for k in T.DEFAULTS} == {k: (F32(v) if isinstance(v, float) else v) for k, v in T.DEFAULTS.items()}
    assert pcr.TreeBandConfig("hag_1", "ids").id_band_name == "ids"
    base = run_pipeline(G.pipeline_cfg(W, H, CPU, radius=RADIUS), clouds[:1])[0]
    cfg = G.pipeline_cfg(W, H, CPU, radius=RADIUS)
    cfg.trees = []
    same = run_pipeline(cfg, clouds[:1])[0]
    assert same[0] == base[0]
    for a, b in zip(same[1], base[1]):
        M.bits_equal(a, b)
    pipe = pcr.Pipeline.create(cfg)
    with pytest.raises(RuntimeError, match="no trees entry 0"):
        pipe.trees(0)


@pytest.mark.parametrize("radius", [0, RADIUS])
def test_host_pipeline_bands_names_sources_and_file(tmp_path, clouds, radius):
    def cfg_of():
        cfg = G.pipeline_cfg(W, H, CPU, radius=radius)
        t = pcr.TerrainBandConfig()
        t.source_band, t.product = "dtm", pcr.TerrainProduct.SlopeDegrees
        cfg.terrain = [t]
        return cfg
    base = run_pipeline(cfg_of(), clouds)
    cfg = cfg_of()
    kw = dict(min_height=0.5, min_crown_height=0.25, window_base=5.0)
    cfg.trees = [T.band_cfg("hag", **kw), T.band_cfg("value_1", "canopy ids", "canopy tops"), T.band_cfg("dtm", min_height=-100.0)]
    cfg.output_path = str(tmp_path / "t.tif")
    got = run_pipeline(cfg, clouds)
    new = ["hag_tree_id", "hag_tree_height", "canopy ids", "canopy tops", "dtm_tree_id", "dtm_tree_height"]
    for k in range(2):                                     # (k = 1: a second finalize() after another ingest is right again)
        names, bands, tables = got[k]
        assert names == base[k][0] + new                   # behind the terrain band
        for b in range(6):
            M.bits_equal(bands[b], base[k][1][b], f"band {b} is what it was")
        src = dict(zip(names, bands))
        for e, t in enumerate(cfg.trees):                  # from the source as it leaves the pipeline: filled
            want = T.host(src[t.source_band], T.spec_of(t))
            del want["table"]["x"], want["table"]["y"]      # (the pipeline's are by its geometry: below)
            T.same_result(dict(id=bands[6 + 2 * e], height=bands[7 + 2 * e], table=tables[e]), want, names[6 + 2 * e])
        m = T.model(src["hag"], **kw)
        del m["table"]["x"], m["table"]["y"]
        T.same_result(dict(id=bands[6], height=bands[7], table=tables[0]), m, "model")
        assert len(tables[0]["row"]) >= 2
        assert tables[1]["x"].tolist() == [c + 0.5 for c in tables[1]["col"]]
        assert tables[1]["y"].tolist() == [float(H) - (r + 0.5) for r in tables[1]["row"]]
        if radius:
            assert np.isnan(bands[10]).any(), "tree bands are not filled"
    assert not np.array_equal(got[0][1][6], got[1][1][6], equal_nan=True)
    assert pcr.read_geotiff_band_names(cfg.output_path) == got[1][0]
    for b, band in enumerate(got[1][1]):
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), band, f"file band {b}")


def test_create_errors():
    def refused(entries, **kw):
        cfg = G.pipeline_cfg(W, H, kw.pop("mode", CPU), **kw)
        t = pcr.TerrainBandConfig()
        t.source_band, t.product = "dtm", pcr.TerrainProduct.SlopeDegrees
        cfg.terrain = [t] if kw.get("ground", True) else []
        cfg.trees = entries
        assert pcr.Pipeline.create(cfg) is None
        return pcr.pipeline_create_error()
    ok = T.band_cfg("hag")
    assert refused([ok, T.band_cfg("z_2")]) == "pipeline: trees[1].source_band 'z_2' names no source band of the result"
    assert refused([T.band_cfg("")]) == "pipeline: trees[0].source_band '' names no source band of the result"
    assert "trees[0].source_band 'dtm_slope' names no source band" in refused([T.band_cfg("dtm_slope")])        # a terrain band
    assert "trees[1].source_band 'hag_tree_id' names no source band" in refused([ok, T.band_cfg("hag_tree_id")])  # a tree band
    assert "trees[0].source_band 'hag'" in refused([ok], top=False)
    assert refused([ok, T.band_cfg("hag")]) == "pipeline: trees[1].id_band_name 'hag_tree_id' clashes with another band"
    assert refused([T.band_cfg("hag", "dtm")]) == "pipeline: trees[0].id_band_name 'dtm' clashes with another band"
    assert refused([T.band_cfg("hag", "a", "dtm_slope")]) == "pipeline: trees[0].height_band_name 'dtm_slope' clashes with another band"
    assert refused([T.band_cfg("hag", "a", "a")]) == "pipeline: trees[0].height_band_name 'a' clashes with another band"
    assert refused([T.band_cfg("hag", f"i{k}", f"h{k}") for k in range(5)]) == "pipeline: trees: more than 4 entries"
    for kw, msg in BAD_SPECS:
        assert refused([ok, T.band_cfg("dtm", **kw)]).startswith("pipeline: trees[1]." + msg)
    for mode in (CPU, pcr.ExecutionMode.GPU):
        cfg = G.pipeline_cfg(W, H, mode, ground=False)
        cfg.trees = [T.band_cfg("value_1")]
        cfg.shard_row_begin, cfg.shard_row_end = 16, 32
        assert pcr.Pipeline.create(cfg) is None
        assert pcr.pipeline_create_error() == "pipeline: tree bands need the whole grid; derive them from the gathered grid with segment_trees"
