"""Polygonize without a GPU: the host twin (pcr_hip_polygonize_host, a sequential trace) against the brute-force model of the
contract (tests/polygonize_common.py), through the C-ABI and through pcr.polygonize; what every ring table must satisfy; the round
trip through rasterize_polygons on four geometries; every refusal; the empty set; Pipeline.polygonize on the host engine; the
chain from a canopy to crown outlines; the WKT and GeoJSON writers; the exports."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import pcr
import polygonize_common as P
import rasterize_common as R
import trees_common as T
import zonal_common as Z
from conftest import load_cabi

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def rectangle():
    band = np.full((5, 4431), np.nan, F32)
    band[1:4, 1:4430] = 9
    return band


CASES = {
    "1 x 1": lambda: np.ones((1, 1), F32), "1 x 7": lambda: P.blobs(1, 7, 5, nothing=0.2), "7 x 1": lambda: P.blobs(7, 1, 5, nothing=0.2),
    "33 x 65": lambda: P.blobs(33, 65, 5), "70 x 130": lambda: P.blobs(70, 130, 8),
    "checkerboard, two zones": lambda: P.checkerboard(21, 30, True), "checkerboard, one zone": lambda: P.checkerboard(21, 30, False),
    "serpentine": lambda: P.serpentine(65), "rectangle": rectangle, "nested": P.nested, "values": P.values_band,
    "one zone to the edge": lambda: np.full((6, 9), 16777216, F32),
}
MODELS = {}


def case(name):
    """(band, the model's table), made once."""
    if name not in MODELS:
        band = CASES[name]()
        MODELS[name] = (band, P.model(band))
    return MODELS[name]


# ---- 1, 2: the host twin is the model, and the model's rings are what the contract says they are -----------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_model(A, name):
    band, m = case(name)
    P.same_table(P.host_cabi(A, band), m, name)
    P.same_table(P.host_cabi(A, band, stride=band.shape[1] + 5, offset=3), m, name + ", strided")
    P.check_structure(m, band, name)
    g = P.geom(band.shape[1], band.shape[0], 2)
    P.bits_equal(pcr.polygonize(P.make_grid(pcr, band), 0, g.config()), P.set_of(m, g), name + ", pcr.polygonize")


def test_known_answers():
    _, m = case("nested")
    zone1 = [j for j, z in enumerate(m["ring_zone"]) if z == 1]
    assert len(zone1) == 5 and int((m["ring_zone"] == 2).sum()) == 2 and int((m["ring_zone"] == 3).sum()) == 2
    assert m["ring_offset"][1] - m["ring_offset"][0] == 8                    # the big square and the notch in its left side
    _, m = case("serpentine")
    assert len(m["ring_zone"]) == 1 and m["E"] == 2 * (33 * 65 + 32) + 2 > 4000      # a path of N cells has 2 N + 2 sides
    _, m = case("rectangle")
    assert m["E"] == 2 * (3 + 4429) and m["vertex_row"].tolist() == [1, 1, 4, 4] and m["vertex_col"].tolist() == [1, 4430, 4430, 1]
    _, m = case("values")
    assert sorted(set(m["ring_zone"].tolist())) == [1, 16777216]
    band, m = case("checkerboard, one zone")
    assert m["E"] == 4 * 315 == 4 * len(m["ring_zone"]) and (np.diff(m["ring_offset"]) == 4).all()
    s = pcr.polygonize(P.make_grid(pcr, band, P.geom(30, 21)))
    assert s.num_polygons == 1 and s.num_rings == 315 and s.values.tolist() == [1.0]
    # ring keys ascend: the first vertex of a ring is the start corner of its smallest corner slot
    key = m["vertex_row"][m["ring_offset"][:-1]].astype(np.int64) * 31 + m["vertex_col"][m["ring_offset"][:-1]]
    assert (np.diff(key) > 0).all()


# ---- 3: the round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_burning_the_polygons_back_gives_the_band(k):
    P.centres_strictly_inside(P.geom(130, 70, k))
    for name in ("70 x 130", "33 x 65", "checkerboard, two zones", "nested", "values", "serpentine"):
        band, _ = case(name)
        g = P.geom(band.shape[1], band.shape[0], k)
        P.centres_strictly_inside(g)
        s = pcr.polygonize(P.make_grid(pcr, band, g))
        back = pcr.rasterize_polygons(s, g.config(), background=R.nan32())
        R.bits_equal(np.array(back.band_array(0)), P.burn_target(band), f"{name}, geometry {k}")


# ---- 4: refusals, the empty set, the host engine ---------------------------------------------------------------------------------
def test_cabi_refusals_need_no_gpu(A):
    L = A.lib()
    w, h = 16, 8
    band = np.ones(4096, F32)
    n, m = C.c_size_t(0), C.c_size_t(0)
    err = lambda: L.pcr_hip_last_error().decode()
    assert L.pcr_hip_polygonize_cells_work_bytes(w, h, C.byref(n)) == 0 and 2 * w * h <= n.value <= 2 * w * h + 1024
    assert L.pcr_hip_polygonize_cells_work_bytes(0, h, C.byref(n)) == 1 and "width and height must be positive" in err()
    assert L.pcr_hip_polygonize_cells_work_bytes(w, h, None) == 1 and "null argument" in err()
    assert L.pcr_hip_polygonize_cells_work_bytes(32768, 32768, C.byref(n)) == 1 and "more than 2^30 - 1 cells" in err()
    assert L.pcr_hip_polygonize_cells_work_bytes(32768, 32767, C.byref(n)) == 0
    assert L.pcr_hip_polygonize_cells_work_bytes(w, h, C.byref(n)) == 0
    assert L.pcr_hip_polygonize_rings_work_bytes(100, C.byref(m)) == 0 and 29 * 100 <= m.value <= 29 * 100 + 64
    assert L.pcr_hip_polygonize_rings_work_bytes(-1, C.byref(m)) == 1 and "n_edges" in err()
    assert L.pcr_hip_polygonize_rings_work_bytes(100, None) == 1 and "null argument" in err()
    assert L.pcr_hip_polygonize_rings_work_bytes(100, C.byref(m)) == 0
    cells, rings = np.zeros(n.value + 64, np.uint8), np.zeros(m.value + 64, np.uint8)
    outs = [np.zeros(256, np.int64) for _ in range(4)]
    bp, cp, rp = band.ctypes.data, cells.ctypes.data, rings.ctypes.data

    def edges(msg, b=bp, w_=w, h_=h, st=w, c=cp, cb=None):
        assert L.pcr_hip_polygonize_edges(b, w_, h_, st, c, n.value if cb is None else cb, None) == 1, msg
        assert msg in err(), err()

    def host(msg, b=bp, w_=w, h_=h, st=w):
        e = C.c_int64(0)
        assert L.pcr_hip_polygonize_host(b, w_, h_, st, C.byref(e), None, None, 0, 0, None, None, None, None) == 1, msg
        assert msg in err(), err()

    for refuse in (edges, host):                                     # the same message on both paths
        refuse("polygonize: null argument", b=None)
        refuse("polygonize: width and height must be positive", w_=0)
        refuse("polygonize: width and height must be positive", h_=-1)
        refuse("polygonize: stride smaller than width", st=w - 1)
        refuse("polygonize: more than 2^30 - 1 cells", w_=32768, h_=32768, st=32768)
    edges("polygonize: null argument", c=None)
    edges("cells_work_bytes too small", cb=n.value - 1)
    edges("the cell work area overlaps the band", c=bp + 64)

    def rings_(msg, E=100, c=cp, r=rp, rb=None, b=bp):
        assert L.pcr_hip_polygonize_rings(b, w, h, w, c, n.value, E, r, m.value if rb is None else rb, None, None) == 1, msg
        assert msg in err(), err()

    rings_("polygonize: null argument", r=None)
    rings_("n_edges must be between 1 and 4 per cell", E=0)
    rings_("n_edges must be between 1 and 4 per cell", E=4 * w * h + 1)
    rings_("rings_work_bytes too small", rb=m.value - 1)
    rings_("the ring work area overlaps the band", r=bp + 128)
    rings_("the work areas overlap", r=cp + 16, c=cp)

    def fetch(msg, Rn=10, V=40, z=outs[0].ctypes.data, o=outs[1].ctypes.data, vr=outs[2].ctypes.data, vc=outs[3].ctypes.data):
        assert L.pcr_hip_polygonize_fetch(bp, w, h, w, cp, n.value, 100, rp, m.value, Rn, V, z, o, vr, vc, None) == 1, msg
        assert msg in err(), err()

    fetch("polygonize: null argument", vc=None)
    fetch("n_rings and n_vertices must be between 1 and n_edges", Rn=0)
    fetch("n_rings and n_vertices must be between 1 and n_edges", V=101)
    fetch("an output overlaps an input, a work area or another output", z=bp)
    fetch("an output overlaps an input, a work area or another output", o=rp + 8)
    fetch("an output overlaps an input, a work area or another output", vr=outs[3].ctypes.data + 4)
    e = C.c_int64(0)
    assert L.pcr_hip_polygonize_host(bp, w, h, w, C.byref(e), None, None, -1, 0, None, None, None, None) == 1 and "capacity" in err()
    assert L.pcr_hip_polygonize_count(None, n.value, C.byref(e), None, None, None, None, None) == 1 and "null argument" in err()
    assert L.pcr_hip_polygonize_count(cp, 8, C.byref(e), None, None, None, None, None) == 1 and "too small" in err()


def test_the_twin_writes_no_partial_table(A):
    L = A.lib()
    band, m = case("nested")
    h, w = band.shape
    Rn, V = len(m["ring_zone"]), len(m["vertex_row"])
    zone, off = np.full(Rn, 77, np.uint32), np.full(Rn + 1, 77, np.int64)
    row, col = np.full(V, 77, np.int32), np.full(V, 77, np.int32)
    counts = [C.c_int64(-1) for _ in range(3)]
    A.check(L.pcr_hip_polygonize_host(band.ctypes.data, w, h, w, *[C.byref(c) for c in counts], Rn, V - 1, zone.ctypes.data, off.ctypes.data,
                                      row.ctypes.data, col.ctypes.data))
    assert [c.value for c in counts] == [m["E"], Rn, V] and (zone == 77).all() and (off == 77).all() and (row == 77).all()
    A.check(L.pcr_hip_polygonize_host(band.ctypes.data, w, h, w, None, None, None, Rn, V, zone.ctypes.data, off.ctypes.data, row.ctypes.data,
                                      col.ctypes.data))
    P.same_table(dict(E=m["E"], ring_zone=zone, ring_offset=off, vertex_row=row, vertex_col=col), m, "the table when it fits")


def test_the_empty_set_and_the_refusals_of_pcr_polygonize():
    nothing = np.array([0x7FC00000, 0xFFC00001], np.uint32).view(F32)[np.arange(63) % 2].reshape(7, 9)
    s = pcr.polygonize(P.make_grid(pcr, nothing, P.geom(9, 7)))
    assert s.num_polygons == 0 and s.num_rings == 0 and s.num_vertices == 0
    assert s.ring_offsets.tolist() == [0] and s.polygon_offsets.tolist() == [0] and s.coords.shape == (0, 2)
    assert s.to_wkt() == []
    band, _ = case("nested")
    grid = P.make_grid(pcr, band)
    with pytest.raises(RuntimeError, match="polygonize: the grid has no geometry"):
        pcr.polygonize(grid)
    with pytest.raises(RuntimeError, match="polygonize: the geometry's width and height are not the grid's"):
        pcr.polygonize(grid, 0, P.geom(20, 17).config())
    for b in (-1, 1):
        with pytest.raises(RuntimeError, match="polygonize: band index outside the grid"):
            pcr.polygonize(grid, b, P.geom(20, 16).config())
    d = pcr.BandDesc()
    d.name, d.dtype = "ids", pcr.DataType.Int32
    with pytest.raises(RuntimeError, match="polygonize: the band must be Float32"):
        pcr.polygonize(pcr.Grid.create(8, 8, [d]), 0, P.geom(8, 8).config())
    grid.set_geometry(P.geom(20, 16, 1).config())                    # the grid's own geometry, and one given over it
    P.bits_equal(pcr.polygonize(grid), P.set_of(case("nested")[1], P.geom(20, 16, 1)), "the grid's own geometry")
    P.bits_equal(pcr.polygonize(grid, grid_config=P.geom(20, 16, 2).config()), P.set_of(case("nested")[1], P.geom(20, 16, 2)), "a given one")


def test_pipeline_polygonize_on_the_host_engine():
    W, H = 70, 40
    cfg = Z.pipeline_cfg(pcr, W, H, pcr.ExecutionMode.CPU)
    pipe = Z.create(pcr, cfg, "host")
    stale = "pipeline: polygonize: no band 'value_1_tree_id' \\(of a finalize with no ingest since\\)"
    with pytest.raises(RuntimeError, match=stale):
        pipe.polygonize("value_1_tree_id")
    pipe.ingest(Z.canopy_points(pcr, W, H, 1, extra=2000))
    with pytest.raises(RuntimeError, match=stale):
        pipe.polygonize("value_1_tree_id")
    pipe.finalize()
    s = pipe.polygonize("value_1_tree_id")
    with pytest.raises(RuntimeError, match="pipeline: polygonize: 'crowns' names no Float32 band of the result"):
        pipe.polygonize("crowns")
    res = pipe.result()
    ids = np.array(res.band_array(res.band_index("value_1_tree_id")))
    P.bits_equal(s, pcr.polygonize(res, res.band_index("value_1_tree_id")), "Pipeline.polygonize against pcr.polygonize of the result")
    P.bits_equal(s, P.set_of(P.model(ids), R.Geom(W, H)), "... and against the model")
    crowns = np.unique(P.zones_of(ids))
    assert s.values.tolist() == crowns[crowns > 0].tolist() and s.num_polygons > 5
    table = pipe.zonal(0)                                            # a polygon of value z belongs to the table's row z - 1
    assert table["zone"][s.values.astype(int) - 1].tolist() == s.values.tolist()
    R.bits_equal(np.array(pcr.rasterize_polygons(s, cfg.grid).band_array(0)), P.burn_target(ids), "crowns burnt back")
    pipe.ingest(Z.canopy_points(pcr, W, H, 1, extra=2000))
    with pytest.raises(RuntimeError, match=stale):
        pipe.polygonize("value_1_tree_id")
    pipe.finalize()
    assert pipe.polygonize("value_1_tree_id").num_polygons > 5
    shard = Z.pipeline_cfg(pcr, W, H, pcr.ExecutionMode.CPU)
    shard.trees, shard.zonal, shard.cell_stats, shard.histograms = [], [], [], []
    shard.shard_row_begin, shard.shard_row_end = 0, 20
    sp = pcr.Pipeline.create(shard)
    if sp is not None:                                               # (an engine that takes row-block shards)
        sp.ingest(Z.canopy_points(pcr, W, H, 1, extra=2000))
        sp.finalize()
        with pytest.raises(RuntimeError, match="pipeline: polygonize: not on a row-block shard"):
            sp.polygonize("value_1")


# ---- 5: the chain ------------------------------------------------------------------------------------------------------------------
def test_crowns_of_a_canopy_as_polygons():
    z = T.canopy(65, 33, 4)
    g = P.geom(65, 33, 1)
    grid, table = pcr.segment_trees(P.make_grid(pcr, z, g), 0)
    ids = np.array(grid.band_array(0))
    grid.set_geometry(g.config())
    s = pcr.polygonize(grid, 0)
    assert s.num_polygons == len(np.unique(ids[~np.isnan(ids)])) > 5
    R.bits_equal(np.array(pcr.rasterize_polygons(s, g.config()).band_array(0)), P.burn_target(ids), "the id band burnt back")
    P.check_structure(P.model(ids), ids, "crowns")


# ---- 6: the writers ----------------------------------------------------------------------------------------------------------------
def writer_case():
    """Polygon 1: a shell with a hole, an island in the hole, and a second part; polygon 2: one ring."""
    a = np.full((12, 16), np.nan, F32)
    a[1:10, 1:10] = 1
    a[3:8, 3:8] = np.nan
    a[4:7, 4:7] = 1
    a[2:5, 12:15] = 1
    a[10:12, 11:16] = 2
    return a


@pytest.mark.parametrize("k", range(4))
def test_writers_read_back_to_the_same_grid(tmp_path, k):
    band = writer_case()
    g = P.geom(16, 12, k)
    s = pcr.polygonize(P.make_grid(pcr, band, g))
    assert s.num_polygons == 2 and s.num_rings == 5
    want = np.array(pcr.rasterize_polygons(s, g.config()).band_array(0))
    R.bits_equal(want, P.burn_target(band), "the set itself")
    texts = s.to_wkt()
    assert texts[0].startswith("MULTIPOLYGON (((") and texts[1].startswith("POLYGON ((") and len(texts) == 2
    R.bits_equal(np.array(pcr.rasterize_polygons(pcr.PolygonSet.from_wkt(texts, s.values), g.config()).band_array(0)), want, "WKT")
    path = str(tmp_path / "crowns.geojson")
    props = {"cells": np.array([74, 10], np.int64), "mean": np.array([1.5, np.nan], F32), "name": ["a", "b"]}
    pcr.write_geojson_polygons(path, s, props)
    back = pcr.read_geojson_polygons(path, "value")
    assert back.values.tolist() == [1.0, 2.0] and back.num_rings == 5
    R.bits_equal(np.array(pcr.rasterize_polygons(back, g.config()).band_array(0)), want, "GeoJSON")
    doc = json.load(open(path))
    f0, f1 = doc["features"]
    assert f0["properties"] == {"value": 1.0, "cells": 74, "mean": 1.5, "name": "a"}
    assert f1["properties"] == {"value": 2.0, "cells": 10, "mean": None, "name": "b"}
    assert f0["geometry"]["type"] == "MultiPolygon" and f1["geometry"]["type"] == "Polygon"
    # shells and holes: the outer square holds the hole, the island and the far part are shells of their own
    parts = sorted(f0["geometry"]["coordinates"], key=len)
    assert [len(p) for p in parts] == [1, 1, 2]

    def area2(ring):
        r = np.array(ring, F64)
        assert (r[0] == r[-1]).all() and len(r) >= 5
        d = r - r[0]
        return float(np.sum(d[:-1, 0] * d[1:, 1] - d[1:, 0] * d[:-1, 1]))

    cell = abs(float(g.csx) * float(g.csy))
    assert sorted(round(area2(p[0]) / (2 * cell)) for p in parts) == [9, 9, 81]          # shells counter-clockwise: positive
    assert round(area2(parts[2][1]) / (2 * cell)) == -25                                  # the hole clockwise
    assert round(area2(f1["geometry"]["coordinates"][0]) / (2 * cell)) == 10
    with pytest.raises(ValueError, match="property 'cells' has 3 entries for 2 polygons"):
        pcr.write_geojson_polygons(path, s, {"cells": [1, 2, 3]})


def test_writers_on_one_ring_and_on_thousands():
    s = pcr.polygonize(P.make_grid(pcr, np.full((2, 3), 4, F32), P.geom(3, 2)))
    assert s.to_wkt() == ["POLYGON ((0.0 0.0, 3.0 0.0, 3.0 2.0, 0.0 2.0, 0.0 0.0))"]         # counter-clockwise, closed
    band, _ = case("checkerboard, one zone")
    g = P.geom(30, 21)
    s = pcr.polygonize(P.make_grid(pcr, band, g))
    texts = s.to_wkt()
    assert len(texts) == 1 and texts[0].count("((") == 315
    R.bits_equal(np.array(pcr.rasterize_polygons(pcr.PolygonSet.from_wkt(texts), g.config()).band_array(0)), P.burn_target(band), "315 shells")


# ---- 7: the exports ----------------------------------------------------------------------------------------------------------------
def test_exports(A):
    text = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    assert "polygonize" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(pcr_hip_[a-z0-9_]+)\s*\(", text)))
    assert sorted(A.SYMBOLS) == names
    lib = C.CDLL(A.LIB_PATH)
    for name in ("pcr_hip_polygonize_cells_work_bytes", "pcr_hip_polygonize_rings_work_bytes", "pcr_hip_polygonize_edges",
                 "pcr_hip_polygonize_count", "pcr_hip_polygonize_rings", "pcr_hip_polygonize_fetch", "pcr_hip_polygonize_host"):
        assert name in names and hasattr(lib, name), name
    assert A.lib().pcr_hip_abi_version() == 5
    assert C.sizeof(A.PolygonizeParams) == 32
