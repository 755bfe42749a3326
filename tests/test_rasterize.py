"""Polygons burnt into a label band, without a GPU: the C-ABI's host twin, pcr.rasterize_polygons on Host and the host engine's
set_zones(name, polygons), each BIT FOR BIT against the brute-force model of the contract (tests/rasterize_common.py: every cell
against every edge in NumPy float64 scalars); known answers, the half-open rule, overlap, a partition with shared wiggly edges,
grids of every sign, the edges of the domain, every refusal with its message, the WKT and GeoJSON parsers, and the composition
with the zonal tables."""
import ctypes as C
import json

import numpy as np
import pytest

import pcr
import rasterize_common as R
import zonal_common as Z
from conftest import load_cabi

F32, F64 = np.float32, np.float64
CPU = pcr.ExecutionMode.CPU
UNIT8 = R.Geom(8, 8)


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def both(A, polys, geom, what, background=None):
    """The host twin (strided, between sentinels) and pcr.rasterize_polygons on Host against the model; -> the band."""
    want = R.model(polys, geom, background)
    R.bits_equal(R.host_cabi(A, polys, geom, background, stride=geom.w + 5, offset=3), want, what + ": host twin")
    kw = {} if background is None else dict(background=background)
    grid = pcr.rasterize_polygons(polys.to_pcr(), geom.config(), **kw)
    assert grid.num_bands() == 1 and grid.band_desc(0).name == "label" and grid.location() == pcr.MemoryLocation.Host
    assert (grid.cols(), grid.rows()) == (geom.w, geom.h)
    R.bits_equal(np.array(grid.band_array(0)), want, what + ": pcr.rasterize_polygons")
    return want


def test_centres_are_cell_to_world():
    for geom in (UNIT8, R.Geom(70, 130, min_x=-3.25, max_y=140.7, csx=1.3, csy=-1.1), R.Geom(9, 7, 1e6 + 0.3, 5e6 + 0.7, -0.37, 0.21)):
        g = geom.config()
        for c, r in ((0, 0), (3, 5), (geom.w - 1, geom.h - 1)):
            x, y = g.cell_to_world(c, r)
            assert F64(x).tobytes() == geom.cx(c).tobytes() and F64(y).tobytes() == geom.cy(r).tobytes()


def test_known_answers(A):
    m = both(A, R.Polys([[R.rect(2, 2, 6, 6)]]), UNIT8, "square")
    assert int((m == 1).sum()) == 16 and (m[2:6, 2:6] == 1).all()
    # vertices ON cell centres: closed on the low-x and low-y sides, open on the high ones -- centres 2.5, 3.5, 4.5, never 5.5
    m = both(A, R.Polys([[R.rect(2.5, 2.5, 5.5, 5.5)]]), UNIT8, "centred square")
    rows, cols = np.nonzero(m == 1)
    assert int((m == 1).sum()) == 9
    assert sorted(set(UNIT8.cx(c) for c in cols)) == [2.5, 3.5, 4.5] and sorted(set(UNIT8.cy(r) for r in rows)) == [2.5, 3.5, 4.5]
    outer, inner = R.rect(1, 1, 7, 7), R.rect(3, 3, 5, 5)
    m = both(A, R.Polys([[outer, inner]]), UNIT8, "donut")
    assert int((m == 1).sum()) == 36 - 4 and np.isnan(m[3:5, 3:5]).all()
    for ring in (outer, outer[::-1]):
        for hole in (inner, inner[::-1]):
            R.bits_equal(R.host_cabi(A, R.Polys([[ring, hole]]), UNIT8), m, "winding")
    # a MULTIPOLYGON's parts are further rings of one polygon
    m = both(A, R.Polys([[R.rect(0, 0, 2, 2), R.rect(5, 5, 8, 8)]]), UNIT8, "two parts")
    assert int((m == 1).sum()) == 4 + 9


def test_overlap_the_greatest_index_wins(A):
    polys = R.Polys([[R.rect(1, 1, 6, 6)], [R.rect(3, 3, 8, 8)], [R.rect(0, 4, 4, 8)]], values=[7.5, -2.0, 0.25])
    m = both(A, polys, UNIT8, "overlap")
    # (row r is y = 7.5 - r): all three, the first two, the first and the third, the first alone
    assert m[3, 3] == F32(0.25) and m[3, 4] == F32(-2.0) and m[4, 3] == F32(-2.0) and m[3, 1] == F32(0.25) and m[6, 1] == F32(7.5)
    # the same polygons in another order of the SET give another band: the index decides, not the order of execution
    m2 = both(A, polys.subset([2, 1, 0]), UNIT8, "overlap, reversed set")
    assert m2[3, 3] == F32(7.5)


def test_partition_labels_every_cell_once(A):
    geom = R.Geom(40, 30, min_x=100.0, max_y=530.0)
    parts = R.partition(100.0, 500.0, 140.0, 530.0, 4, 3, seed=5)
    n = len(parts)
    values = np.arange(n, dtype=F32) * 3 + 1
    polys = R.Polys(parts, values)
    m = both(A, polys, geom, "partition")
    assert not np.isnan(m).any() and sorted(set(m.ravel().tolist())) == values.tolist()
    order = list(range(n))[::-1]
    R.bits_equal(R.host_cabi(A, polys.subset(order), geom), m, "reversed order, same values")
    cover = np.zeros((geom.h, geom.w), np.int64)
    for p in range(n):
        cover += ~np.isnan(R.host_cabi(A, polys.subset([p]), geom))
    assert (cover == 1).all(), "each cell centre belongs to exactly one polygon of the partition"


@pytest.mark.parametrize("csx, csy, min_x, max_y", [(1.3, -1.1, -3.25, 70.7), (-1.3, -1.1, 48.5, 70.7), (1.3, 1.1, -3.25, -2.2),
                                                    (-0.7, 0.9, 30.1, 1.6)])
def test_grids_of_every_sign(A, csx, csy, min_x, max_y):
    geom = R.Geom(37, 61, min_x=min_x, max_y=max_y, csx=csx, csy=csy)
    polys = R.Polys(R.partition(0, 0, 45, 66, 3, 4, 3) + [R.donut(20, 30, 14, 6), [R.ngon(22.5, 31.5, 4.0, 4, phase=0.0)]])
    m = both(A, polys, geom, f"cell sizes {csx}, {csy}")
    assert 100 < int((~np.isnan(m)).sum())


def test_edges_of_the_domain(A):
    geom = R.Geom(20, 12)
    partly = R.ngon(0.0, 6.0, 5.0, 9)                                    # crossings left of column 0
    right = R.ngon(20.0, 3.0, 4.5, 7)                                    # ... and right of the last column
    outside = R.rect(40, 40, 50, 50)
    flat = np.array([[2, 2], [9, 2], [5, 2]], F64)                       # zero area
    spike = np.array([[3, 3], [8, 9], [3, 3.0]], F64)
    closed = np.concatenate([R.rect(10, 5, 15, 10), [[10, 5]]])          # the closing vertex repeated
    between = R.rect(4.6, 0.6, 5.4, 1.4)                                 # between the centres: no cell
    huge = R.rect(-1e100, -1e100, 1e100, 1e100)
    polys = R.Polys([[huge], [partly], [right], [outside], [flat], [spike], [closed], [between]])
    m = both(A, polys, geom, "domain")
    assert not np.isnan(m).any() and set(m.ravel().tolist()) == {1.0, 2.0, 3.0, 7.0}
    R.bits_equal(R.host_cabi(A, R.Polys([[closed]]), geom), R.host_cabi(A, R.Polys([[closed[:-1]]]), geom), "closing vertex")
    none = both(A, R.Polys([[outside], [flat], [between]]), geom, "nothing labelled")
    assert np.isnan(none).all()
    m = both(A, R.Polys([[partly]], values=[np.float32(np.inf)]), geom, "background", background=-9999.0)
    assert set(m.ravel().tolist()) == {-9999.0, np.inf}
    # no polygon, and a polygon of no ring
    empty = pcr.PolygonSet(np.zeros((0, 2)), np.array([0]), np.array([0]))
    assert np.isnan(np.array(pcr.rasterize_polygons(empty, geom.config()).band_array(0))).all()
    ringless = pcr.PolygonSet(R.rect(1, 1, 5, 5), np.array([0, 4]), np.array([0, 0, 1]))
    assert set(np.array(pcr.rasterize_polygons(ringless, geom.config(), background=0.0).band_array(0)).ravel().tolist()) == {0.0, 2.0}


def test_many_crossings_and_many_polygons(A):
    geom = R.Geom(126, 12)
    m = both(A, R.Polys([[R.comb(2.2, 1.3, pitch=3.0)]]), geom, "comb")
    assert max(int((np.diff((~np.isnan(row)).astype(int)) != 0).sum()) for row in m) == 80
    rng = np.random.default_rng(11)
    small = [[R.ngon(rng.uniform(0, 33), rng.uniform(0, 21), rng.uniform(0.6, 3.0), int(rng.integers(3, 9)), rng.uniform(0, 6))]
             for _ in range(60)]
    both(A, R.Polys(small), R.Geom(33, 21), "overlapping n-gons")


def test_refusals(A):
    sq = R.Polys([[R.rect(2, 2, 6, 6)]])
    ptr = lambda a: a.ctypes.data

    def refused(msg, polys=sq, geom=UNIT8, **kw):
        rc, text = R.host_cabi_error(A, polys, geom, **kw)
        assert rc == 1 and text == "rasterize_polygons: " + msg, (rc, text)

    refused("null argument", out=False)
    refused("null argument", params=None)
    refused("null argument", coords=None)
    refused("null or inconsistent offsets", ring_offsets=None)
    refused("null or inconsistent offsets", polygon_offsets=None)
    for ro in ([0, 5], [1, 4], [0, 3]):
        bad = np.array(ro, np.int64)
        refused("null or inconsistent offsets", ring_offsets=ptr(bad))
    two = R.Polys([[R.rect(0, 0, 1, 1)], [R.rect(2, 2, 3, 3)]])
    for ro in ([0, 6, 4, 8], ):
        bad = np.array(ro[:3], np.int64)
        refused("null or inconsistent offsets", polys=two, ring_offsets=ptr(bad))
    bad = np.array([0, 2, 1], np.int64)
    refused("null or inconsistent offsets", polys=two, polygon_offsets=ptr(bad))
    bad = np.array([0, 1, 1], np.int64)
    refused("null or inconsistent offsets", polys=two, polygon_offsets=ptr(bad))
    refused("a negative count", V=-1)
    thin = R.Polys([[R.rect(0, 0, 1, 1)]])
    thin.ring_offsets = np.array([0, 2, 4], np.int64)
    thin.polygon_offsets = np.array([0, 2], np.int64)
    refused("a ring of fewer than 3 vertices", polys=thin)
    for v in (np.nan, np.inf, -np.inf, 1.0000001e100, -2e100):
        p = R.Polys([[R.rect(2, 2, 6, 6)]])
        p.coords[2, 1] = v
        refused("a coordinate is not finite or beyond 1e100", polys=p)
    refused("more than 2^31 - 2 polygons", P=2 ** 31 - 1)
    big = R.Geom(65536, 32768)
    refused("more than 2^31 - 1 cells", geom=big, out_ptr=ptr(np.zeros(8, F32)))
    for field, v in (("min_x", np.nan), ("max_y", np.inf), ("cell_size_x", 0.0), ("cell_size_y", np.nan)):
        g = UNIT8.cabi(A)
        setattr(g, field, v)
        refused("the grid's origin and cell sizes must be finite, the cell sizes not zero", grid=C.byref(g))
    g = UNIT8.cabi(A)
    g.width = 0
    refused("width and height must be positive", grid=C.byref(g))
    refused("out_stride smaller than width", stride=7)
    refused("the output overlaps an input or the work area", out_ptr=ptr(sq.coords))
    L = A.lib()
    n = C.c_size_t(0)
    assert L.pcr_hip_rasterize_work_bytes(4, 1, 8, 8, C.byref(n)) == 0 and n.value >= 8 * 8 * 4 + 4 * 32 + 44
    assert L.pcr_hip_rasterize_work_bytes(4, 1, 65536, 32768, C.byref(n)) == 1
    assert b"more than 2^31 - 1 cells" in L.pcr_hip_last_error()
    # the device entry point refuses the same before any HIP call (there is no device here): too little work memory last
    buf = np.zeros(64 + 64, F32)
    g, p = UNIT8.cabi(A), A.RasterizeParams()
    args = (ptr(sq.coords), 4, ptr(sq.ring_offsets), 1, ptr(sq.polygon_offsets), 1, None, C.byref(p))
    work = np.zeros(16, np.uint8)
    assert L.pcr_hip_rasterize_polygons(C.byref(g), *args, ptr(buf), 8, ptr(work), 16, None) == 1
    assert L.pcr_hip_last_error() == b"rasterize_polygons: work_bytes too small (pcr_hip_rasterize_work_bytes)"
    assert L.pcr_hip_rasterize_polygons(C.byref(g), *args, ptr(buf), 8, ptr(buf) + 64, 1 << 20, None) == 1
    assert L.pcr_hip_last_error() == b"rasterize_polygons: the output overlaps an input or the work area"
    assert L.pcr_hip_rasterize_polygons(C.byref(g), *args, ptr(buf), 8, None, 1 << 20, None) == 1
    assert L.pcr_hip_last_error() == b"rasterize_polygons: null argument"
    # ... and the public interface passes them on
    with pytest.raises(RuntimeError, match="a ring of fewer than 3 vertices"):
        pcr.rasterize_polygons(thin.to_pcr(), UNIT8.config())
    with pytest.raises(RuntimeError, match="null or inconsistent offsets"):
        pcr.rasterize_polygons(pcr.PolygonSet(sq.coords, np.array([0, 3]), np.array([0, 1])), UNIT8.config())
    with pytest.raises(RuntimeError, match="width and height must be positive"):
        pcr.rasterize_polygons(sq.to_pcr(), pcr.GridConfig())
    with pytest.raises(ValueError, match="values must be one per polygon"):
        pcr.PolygonSet(sq.coords, sq.ring_offsets, sq.polygon_offsets, [1.0, 2.0])
    with pytest.raises(ValueError, match="shape"):
        pcr.PolygonSet(np.zeros((4, 3)), sq.ring_offsets, sq.polygon_offsets)


WKT = ["POLYGON ((2 2, 6 2, 6 6, 2 6, 2 2), (3 3, 4 3, 4 4, 3 4, 3 3))",
       "MULTIPOLYGON (((0 0, 1.5 0, 1.5 1.5, 0 1.5, 0 0)), ((6.5 6.5, 8 6.5, 8 8e0, 6.5 8)))",
       "polygon z((1 6 10, 2 6 10, 2 7 10, 1 7 10, 1 6 10))",
       "POLYGON EMPTY"]


def test_wkt_round_trip(A):
    ps = pcr.PolygonSet.from_wkt(WKT)
    assert (ps.num_vertices, ps.num_rings, ps.num_polygons) == (20, 5, 4)
    assert ps.ring_offsets.tolist() == [0, 4, 8, 12, 16, 20] and ps.polygon_offsets.tolist() == [0, 2, 4, 5, 5] and ps.values is None
    want = R.Polys([[R.rect(2, 2, 6, 6), R.rect(3, 3, 4, 4)], [R.rect(0, 0, 1.5, 1.5), R.rect(6.5, 6.5, 8, 8)], [R.rect(1, 6, 2, 7)]])
    assert ps.coords.tobytes() == want.coords.tobytes()
    m = np.array(pcr.rasterize_polygons(ps, UNIT8.config()).band_array(0))
    R.bits_equal(m, R.model(want, UNIT8), "from_wkt")
    assert int((m == 1).sum()) == 15 and int((m == 2).sum()) == 1 + 4 and int((m == 3).sum()) == 1
    assert pcr.PolygonSet.from_wkt(WKT[0], values=[5]).values.tolist() == [5.0]
    for bad in ("POINT (1 2)", "POLYGON ((1 2, 3 4))", "POLYGON ((1 2, 3 x, 5 6))", "POLYGON (1 2, 3 4, 5 6"):
        with pytest.raises(ValueError):
            pcr.PolygonSet.from_wkt([bad])


def test_geojson_round_trip(A, tmp_path):
    sq = [[2, 2], [6, 2], [6, 6], [2, 6], [2, 2]]
    hole = [[3, 3], [4, 3], [4, 4], [3, 4], [3, 3]]
    doc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"plot": 12, "name": "a"}, "geometry": {"type": "Polygon", "coordinates": [sq, hole]}},
        {"type": "Feature", "properties": {"plot": 7.5}, "geometry": {"type": "MultiPolygon", "coordinates": [
            [[[0, 0], [1.5, 0], [1.5, 1.5], [0, 1.5], [0, 0]]], [[[6.5, 6.5, 3.0], [8, 6.5, 3.0], [8, 8, 3.0], [6.5, 8, 3.0]]]]}}]}
    path = tmp_path / "plots.geojson"
    path.write_text(json.dumps(doc))
    ps = pcr.read_geojson_polygons(str(path), value_property="plot")
    assert ps.values.tolist() == [12.0, 7.5] and ps.polygon_offsets.tolist() == [0, 2, 4] and ps.num_vertices == 16
    m = np.array(pcr.rasterize_polygons(ps, UNIT8.config()).band_array(0))
    want = R.Polys([[R.rect(2, 2, 6, 6), R.rect(3, 3, 4, 4)], [R.rect(0, 0, 1.5, 1.5), R.rect(6.5, 6.5, 8, 8)]], values=[12, 7.5])
    R.bits_equal(m, R.model(want, UNIT8), "geojson")
    assert pcr.read_geojson_polygons(str(path)).values is None
    with pytest.raises(ValueError, match="no numeric property 'name'"):
        pcr.read_geojson_polygons(str(path), value_property="name")
    path.write_text(json.dumps(doc["features"][0]["geometry"]))
    assert pcr.read_geojson_polygons(str(path)).num_polygons == 1
    path.write_text(json.dumps({"type": "Feature", "properties": {}, "geometry": {"type": "Point", "coordinates": [1, 2]}}))
    with pytest.raises(ValueError, match="is a Point"):
        pcr.read_geojson_polygons(str(path))


def test_set_zones_from_polygons_on_the_host_engine():
    W, H = 48, 40
    polys = R.Polys(R.partition(2.0, 3.0, 44.0, 37.0, 3, 3, seed=9) + [R.donut(24, 20, 9, 4)])
    tables = []
    for how in ("polygons", "grid"):
        cfg = Z.pipeline_cfg(pcr, W, H, CPU)
        cfg.zonal = [pcr.ZonalConfig("plots", external=True, cell_stats=[0], histograms=[0])]
        pipe = Z.create(pcr, cfg, "host")
        pipe.ingest(Z.canopy_points(pcr, W, H, 1))
        pipe.finalize()
        if how == "polygons":
            with pytest.raises(RuntimeError, match="'stands' names no external label grid"):
                pipe.set_zones("stands", polys.to_pcr())
            with pytest.raises(RuntimeError, match="a ring of fewer than 3 vertices"):
                pipe.set_zones("plots", pcr.PolygonSet(np.zeros((2, 2)), np.array([0, 2]), np.array([0, 1])))
            with pytest.raises(RuntimeError, match="the label grid 'plots' was not set"):
                pipe.zonal(0)
            pipe.set_zones("plots", polys.to_pcr())
        else:
            grid = pcr.rasterize_polygons(polys.to_pcr(), cfg.grid)
            R.bits_equal(np.array(grid.band_array(0)), R.model(polys, R.Geom(W, H)), "the pipeline's grid")
            pipe.set_zones("plots", grid)
        tables.append(pipe.zonal(0))
    assert tables[0]["zone"].tolist() == list(range(1, 11)) and int(tables[0]["cells"].sum()) > 1000
    Z.same_table(tables[0], tables[1], "set_zones(polygons) against set_zones(grid)")
    # no zonal entry: the polygon form refuses like the grid form
    cfg = Z.pipeline_cfg(pcr, W, H, CPU)
    cfg.zonal = []
    with pytest.raises(RuntimeError, match="names no external label grid"):
        Z.create(pcr, cfg, "host").set_zones("plots", polys.to_pcr())


def test_clipping_a_cloud_through_a_label_grid():
    """The README's second composition: the label grid as a Nearest surface channel and a filter on it -- a clip at cell resolution."""
    W, H = 20, 12
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = CPU
    spec = pcr.ReductionSpec()
    spec.value_channel, spec.type = "value", pcr.ReductionType.Count
    cfg.reductions = [spec]
    cfg.surface_channels = [pcr.SurfaceChannelConfig("aoi", mode=pcr.SampleMode.Nearest)]
    cfg.filter.add("aoi", pcr.CompareOp.GreaterEqual, 1.0)
    pipe = Z.create(pcr, cfg, "host")
    polys = R.Polys([[R.ngon(9.0, 6.0, 4.6, 9)], [R.rect(15.0, 1.0, 19.0, 4.0)]])
    label = pcr.rasterize_polygons(polys.to_pcr(), cfg.grid)
    pipe.set_surface("aoi", label, 0)
    rng = np.random.default_rng(2)
    n = 4000
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    cloud = pcr.PointCloud.create(n)
    cloud.set_x_array(x)
    cloud.set_y_array(y)
    cloud.add_channel("value", pcr.DataType.Float32)
    cloud.set_channel_array_f32("value", np.ones(n, F32))
    pipe.ingest(cloud)
    pipe.finalize()
    got = np.array(pipe.result().band_array(0))
    inside = ~np.isnan(R.model(polys, R.Geom(W, H)))
    want = np.zeros((H, W))
    np.add.at(want, (np.floor(H - y).astype(int), np.floor(x).astype(int)), 1.0)
    assert inside.sum() > 60 and (want[inside] > 0).all()
    assert (got[inside] == want[inside]).all(), "every point of a cell inside is kept"
    assert (np.isnan(got[~inside]) | (got[~inside] == 0)).all(), "no point of a cell outside is"
