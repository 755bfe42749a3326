"""Polygon rasterization on the MI355X: pcr_hip_rasterize_polygons through the C-ABI -- grids of one cell, one row, one column,
more than one wave of columns; bounding boxes on both sides of the bitmap's word and of the wave; a box wider than one pass of
the bitmap; rings on both sides of the edge loop's stride; many crossings in one row, holes, hundreds of overlapping polygons,
a partition with shared edges; strided windows between sentinels -- and pcr.rasterize_polygons on Device and the HIP engine's
set_zones(name, polygons).  Everything BIT FOR BIT against the host twin and the host engine, which tests/test_rasterize.py holds
to the brute-force model of the contract."""
import numpy as np
import pytest

import pcr
import rasterize_common as R
import zonal_common as Z
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32 = np.float32
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def same(A, polys, geom, what, background=None):
    """The kernels, contiguous and in a strided window at an element offset, against the host twin; -> the band."""
    want = R.host_cabi(A, polys, geom, background)
    R.bits_equal(R.device_cabi(A, polys, geom, background), want, what)
    R.bits_equal(R.device_cabi(A, polys, geom, background, stride=geom.w + 5, offset=3), want, what + ", strided")
    return want


def mix(h, w, seed):
    """Polygons sized to the grid: a partition under everything, a donut, a triangle with a vertex outside, small n-gons."""
    rng = np.random.default_rng(seed)
    polys = R.partition(-0.5, -0.25, w + 0.5, h + 0.25, max(1, min(4, w // 8)), max(1, min(3, h // 8)), seed)
    polys.append(R.donut(0.55 * w, 0.45 * h, 0.4 * min(w, h) + 0.3, 0.15 * min(w, h)))
    polys.append([np.array([[-3.0, 0.2 * h], [0.7 * w, 1.3 * h], [0.4 * w, 0.1 * h]])])
    for _ in range(6):
        polys.append([R.ngon(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.5, 3.0), int(rng.integers(3, 8)), rng.uniform(0, 6))])
    return R.Polys(polys)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (33, 65), (70, 130)])
def test_grids(A, shape):
    h, w = shape
    geom = R.Geom(w, h)
    polys = mix(h, w, 3)
    m = same(A, polys, geom, f"grid {shape}")
    assert not np.isnan(m).any()
    if shape == (33, 65):                                            # ... and the model itself, once
        R.bits_equal(m, R.model(polys, geom), "host twin against the model")
    for csx, csy, min_x, max_y in ((-1.0, -1.0, float(w), float(h)), (1.0, 1.0, 0.0, 0.0), (-0.7, 0.9, 0.7 * w, 0.05)):
        same(A, polys, R.Geom(w, h, min_x=min_x, max_y=max_y, csx=csx, csy=csy), f"grid {shape}, cell sizes {csx}, {csy}")


@pytest.mark.parametrize("width", [1, 63, 64, 65, 129])
def test_bounding_box_widths(A, width):
    geom = R.Geom(140, 6)
    for x0 in (0.0, 3.0, 9.75):
        if x0 + width > geom.w:
            continue
        box = R.rect(x0, 1.0, x0 + width, 5.0)
        notch = np.array([[x0, 1.0], [x0 + width, 1.0], [x0 + width, 5.0], [x0 + 0.5 * width, 2.2], [x0, 5.0]])
        m = same(A, R.Polys([[box], [notch]], values=[3.0, 4.0]), geom, f"box of {width} columns at {x0}")
        assert int((~np.isnan(m[2])).sum()) == width


def test_a_box_wider_than_one_pass_of_the_bitmap(A):
    w = 4096 + 333                                                   # PCR_HIP_RASTERIZE_BLOCK_COLS and a rest
    geom = R.Geom(w, 3)
    wide = np.array([[1.2, 0.1], [w - 1.3, 0.2], [w - 40.0, 2.9], [4100.4, 1.2], [4090.6, 2.8], [2000.0, 0.9], [30.0, 2.95]])
    holes = [R.rect(x, 0.2, x + 7.3, 2.7) for x in (100.3, 4000.1, 4092.2, 4200.7)]
    polys = R.Polys([[wide] + holes, [R.rect(4095.0, 0.0, 4097.0, 3.0)], [R.comb(4000.4, 0.3, teeth=30, pitch=3.0, depth=1.4, spine=0.4)]])
    m = same(A, polys, geom, "wide box")
    R.bits_equal(m, R.model(polys, geom), "host twin against the model")
    assert {1.0, 2.0, 3.0} <= set(m[~np.isnan(m)].tolist()) and np.isnan(m).any()


@pytest.mark.parametrize("edges", [3, 63, 64, 65, 200])
def test_rings_around_the_edge_loops_stride(A, edges):
    geom = R.Geom(65, 33)
    polys = R.Polys([[R.ngon(31.7, 16.2, 15.5, edges)], [R.ngon(40.0, 12.0, 9.0, edges, phase=1.0), R.ngon(40.0, 12.0, 4.0, edges)]])
    m = same(A, polys, geom, f"{edges} edges")
    assert int((m == 1).sum()) > 100 and int((m == 2).sum()) > 50


def test_comb_donut_overlaps_and_partition(A):
    geom = R.Geom(126, 12)
    m = same(A, R.Polys([[R.comb(2.2, 1.3, pitch=3.0)]]), geom, "comb")
    assert max(int((np.diff((~np.isnan(row)).astype(int)) != 0).sum()) for row in m) == 80
    m = same(A, R.Polys([R.donut(30.0, 25.0, 22.0, 9.5)]), R.Geom(64, 50), "donut")
    assert np.isnan(m[25, 30]) and m[25, 45] == 1
    rng = np.random.default_rng(11)
    small = [[R.ngon(rng.uniform(0, 60), rng.uniform(0, 40), rng.uniform(0.6, 4.0), int(rng.integers(3, 9)), rng.uniform(0, 6))]
             for _ in range(300)]
    m = same(A, R.Polys(small, values=rng.uniform(-5, 5, 300)), R.Geom(60, 40), "300 overlapping n-gons")
    assert np.isnan(m).any() and len(set(m[~np.isnan(m)].tolist())) > 100
    geom = R.Geom(90, 70, min_x=100.0, max_y=570.0)
    parts = R.Polys(R.partition(100.0, 500.0, 190.0, 570.0, 6, 5, seed=5))
    m = same(A, parts, geom, "partition")
    assert not np.isnan(m).any() and len(set(m.ravel().tolist())) == 30
    R.bits_equal(R.device_cabi(A, parts.subset(range(29, -1, -1)), geom), 31.0 - m, "reversed order")


def test_background_and_nothing_to_burn(A):
    geom = R.Geom(33, 9)
    polys = R.Polys([[R.ngon(12.0, 4.0, 3.7, 11)]], values=[np.inf])
    m = same(A, polys, geom, "background", background=-9999.0)
    assert set(m.ravel().tolist()) == {-9999.0, np.inf}
    payload = np.array([0x7FC12345], np.uint32).view(F32)[0]
    m = same(A, polys, geom, "a NaN of another payload", background=payload)
    assert (m.view(np.uint32) == 0x7FC12345).any()
    none = same(A, R.Polys([[R.rect(40, 40, 50, 50)], [np.array([[2, 2], [9, 2], [5, 2.0]])]]), geom, "nothing labelled")
    assert (none.view(np.uint32) == R.NAN_BITS).all()


def test_device_grids_equal_host_grids():
    geom = R.Geom(130, 70, min_x=-3.25, max_y=80.7, csx=1.3, csy=-1.1)
    polys = mix(77, 169, 8)
    host = pcr.rasterize_polygons(polys.to_pcr(), geom.config())
    dev = pcr.rasterize_polygons(polys.to_pcr(), geom.config(), location=pcr.MemoryLocation.Device)
    assert dev.location() == pcr.MemoryLocation.Device and dev.band_desc(0).name == "label"
    R.bits_equal(np.array(dev.to(pcr.MemoryLocation.Host).band_array(0)), np.array(host.band_array(0)), "Device against Host")
    dev = pcr.rasterize_polygons(polys.to_pcr(), geom.config(), background=7.0, location=pcr.MemoryLocation.Device)
    R.bits_equal(np.array(dev.to(pcr.MemoryLocation.Host).band_array(0)),
                 np.array(pcr.rasterize_polygons(polys.to_pcr(), geom.config(), background=7.0).band_array(0)), "background")
    with pytest.raises(RuntimeError, match="a ring of fewer than 3 vertices"):
        pcr.rasterize_polygons(pcr.PolygonSet(np.zeros((2, 2)), np.array([0, 2]), np.array([0, 1])), geom.config(),
                               location=pcr.MemoryLocation.Device)


def test_set_zones_from_polygons_on_the_hip_engine():
    W, H = 70, 40
    polys = R.Polys(R.partition(2.0, 3.0, 66.0, 37.0, 4, 3, seed=9) + [R.donut(35, 20, 9, 4)])
    tables = {}
    for mode, engine in ((CPU, "host"), (GPU, "hip")):
        cfg = Z.pipeline_cfg(pcr, W, H, mode)
        cfg.histograms = []
        cfg.zonal = [pcr.ZonalConfig("plots", external=True, cell_stats=[0])]
        pipe = Z.create(pcr, cfg, engine)
        pipe.ingest(Z.canopy_points(pcr, W, H, 1, extra=2000))
        pipe.finalize()
        with pytest.raises(RuntimeError, match="'stands' names no external label grid"):
            pipe.set_zones("stands", polys.to_pcr())
        pipe.set_zones("plots", polys.to_pcr())
        tables[engine] = pipe.zonal(0)
        if engine == "hip":                                         # ... and again from the grid form, from a Device grid
            pipe.set_zones("plots", pcr.rasterize_polygons(polys.to_pcr(), cfg.grid, location=pcr.MemoryLocation.Device))
            Z.same_table(pipe.zonal(0), tables["hip"], "set_zones(grid) against set_zones(polygons)")
    assert tables["host"]["zone"].tolist() == list(range(1, 14)) and int(tables["host"]["cells"].sum()) > 1500
    Z.same_table(tables["hip"], tables["host"], "the HIP engine against the host engine")
