"""Polygonize on the MI355X: pcr_hip_polygonize_edges / _rings / _fetch through the C-ABI -- grids of one cell, one row, one column,
more than one wave of columns and more than one 1024-cell chunk; checkerboards whose every corner is a saddle, with more rings than
two scan chunks, in many polygons and in one; a ring long enough for more than 12 doubling rounds; runs of thousands of edges
between two corners; nested rings and rings touching at corners; every kind of value that is no zone; strided windows between
sentinels -- and pcr.polygonize on Device and the HIP engine's Pipeline.polygonize.  Everything BIT FOR BIT against the host twin
(a sequential trace, where the kernels double pointers) and the host engine, which tests/test_polygonize.py holds to the
brute-force model of the contract."""
import math

import numpy as np
import pytest

import pcr
import polygonize_common as P
import rasterize_common as R
import zonal_common as Z
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32 = np.float32
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU
DEVICE, HOST = pcr.MemoryLocation.Device, pcr.MemoryLocation.Host


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def same(A, band, what):
    """The kernels, contiguous and in a strided window at an element offset, against the host twin; -> (table, rounds)."""
    want = P.host_cabi(A, band)
    got, key_rounds, rank_rounds = P.device_cabi(A, band)
    P.same_table(got, want, what)
    P.same_table(P.device_cabi(A, band, stride=band.shape[1] + 5, offset=3)[0], want, what + ", strided")
    P.check_structure(got, band, what)
    if want["E"]:
        most = math.ceil(math.log2(want["E"])) + 1
        assert 1 <= key_rounds <= most and 0 <= rank_rounds <= most, (key_rounds, rank_rounds, most)
    return got, key_rounds


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (33, 65), (70, 130)])
def test_grids(A, shape):
    h, w = shape
    band = P.blobs(h, w, 5, nothing=0.2 if h * w > 1 else 0.0)
    t, _ = same(A, band, f"grid {shape}")
    assert t["E"] > 0
    if shape == (33, 65):                                            # ... and the model itself, once
        P.same_table(t, P.model(band), "host twin against the model")
    full = np.full((h, w), 3, F32)                                   # one zone to the band's edge: 4 vertices
    t, _ = same(A, full, f"grid {shape}, one zone")
    assert t["E"] == 2 * (h + w) and t["vertex_row"].tolist() == [0, 0, h, h] and t["vertex_col"].tolist() == [0, w, w, 0]


@pytest.mark.parametrize("two", [True, False])
def test_saddles_everywhere(A, two):
    band = P.checkerboard(70, 130, two)
    t, _ = same(A, band, f"checkerboard, {'two zones' if two else 'one zone'}")
    cells = int((P.zones_of(band) > 0).sum())
    assert t["E"] == 4 * cells and len(t["ring_zone"]) == cells > 2048 and len(t["vertex_row"]) == 4 * cells
    assert set(t["ring_zone"].tolist()) == ({1, 2} if two else {1})


def test_a_long_ring_takes_its_rounds(A):
    band = P.serpentine(65)
    t, key_rounds = same(A, band, "serpentine")
    assert len(t["ring_zone"]) == 1 and t["E"] > 4000
    assert 12 <= key_rounds <= math.ceil(math.log2(t["E"])) + 1, key_rounds


def test_long_runs_between_two_corners(A):
    band = np.full((5, 4431), np.nan, F32)
    band[1:4, 1:4430] = 9
    t, _ = same(A, band, "3 x 4429 rectangle")
    assert t["E"] == 2 * (3 + 4429) and t["vertex_row"].tolist() == [1, 1, 4, 4] and t["vertex_col"].tolist() == [1, 4430, 4430, 1]


def test_nesting_and_corner_touches(A):
    band = P.nested()
    t, _ = same(A, band, "nested")
    P.same_table(t, P.model(band), "nested against the model")
    assert int((t["ring_zone"] == 1).sum()) >= 3 and int((t["ring_zone"] == 3).sum()) == 2


def test_values_that_are_no_zone(A):
    band = P.values_band()
    t, _ = same(A, band, "values")
    assert sorted(set(t["ring_zone"].tolist())) == [1, 16777216]
    nothing = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32).view(F32)[np.arange(33 * 65) % 3].reshape(33, 65)
    t, key_rounds = same(A, nothing, "all NaN")
    assert t["E"] == 0 and len(t["ring_zone"]) == 0 and len(t["vertex_row"]) == 0 and t["ring_offset"].tolist() == [0]


def test_device_grids_equal_host_grids():
    band = P.blobs(70, 130, 8)
    for k in range(4):
        g = P.geom(130, 70, k)
        P.centres_strictly_inside(g)
        host = pcr.polygonize(P.make_grid(pcr, band, g))
        dev = pcr.polygonize(P.make_grid(pcr, band, g).to(DEVICE))
        assert host.num_polygons == 7
        P.bits_equal(dev, host, f"Device against Host, geometry {k}")
        back = pcr.rasterize_polygons(dev, g.config(), location=DEVICE).to(HOST)
        R.bits_equal(np.array(back.band_array(0)), P.burn_target(band), f"burnt back on the device, geometry {k}")
    empty = pcr.polygonize(P.make_grid(pcr, np.full((7, 9), np.nan, F32), P.geom(9, 7)).to(DEVICE))
    assert empty.num_polygons == 0 and empty.num_rings == 0 and empty.num_vertices == 0
    with pytest.raises(RuntimeError, match="polygonize: the grid has no geometry"):
        pcr.polygonize(P.make_grid(pcr, band).to(DEVICE))


@pytest.mark.parametrize("location", [HOST, DEVICE])
def test_pipeline_polygonize_on_the_hip_engine(location):
    W, H = 70, 40
    sets, ids = {}, {}
    for mode, engine in ((CPU, "host"), (GPU, "hip")):
        cfg = Z.pipeline_cfg(pcr, W, H, mode, location if engine == "hip" else None)
        pipe = Z.create(pcr, cfg, engine)
        with pytest.raises(RuntimeError, match="of a finalize with no ingest since"):
            pipe.polygonize("value_1_tree_id")
        pipe.ingest(Z.canopy_points(pcr, W, H, 1, extra=2000))
        pipe.finalize()
        sets[engine] = pipe.polygonize("value_1_tree_id")
        with pytest.raises(RuntimeError, match="'crowns' names no Float32 band"):
            pipe.polygonize("crowns")
        res = pipe.result()
        res = res if res.location() == HOST else res.to(HOST)
        ids[engine] = np.array(res.band_array(res.band_index("value_1_tree_id")))
        if engine == "hip":                                          # the chain, burnt back where the band lives
            back = pcr.rasterize_polygons(sets["hip"], cfg.grid, location=DEVICE).to(HOST)
            R.bits_equal(np.array(back.band_array(0)), P.burn_target(ids["hip"]), "crowns burnt back on the device")
            pipe.ingest(Z.canopy_points(pcr, W, H, 1, extra=2000))
            with pytest.raises(RuntimeError, match="of a finalize with no ingest since"):
                pipe.polygonize("value_1_tree_id")
    R.bits_equal(ids["hip"], ids["host"], "the id bands")
    crowns = np.unique(P.zones_of(ids["host"]))
    assert sets["host"].values.tolist() == crowns[crowns > 0].tolist() and sets["host"].num_polygons > 5
    P.bits_equal(sets["hip"], sets["host"], "the HIP engine against the host engine")
