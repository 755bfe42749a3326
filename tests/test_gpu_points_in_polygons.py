"""The exact point-in-polygon test on the MI355X: k_points_in_polygons through the C-ABI -- counts on both sides of the wave, the
workgroup and the 16-byte quad; x, y and out on 16 bytes and one element off them, out between sentinels; the lattice of
tests/points_in_polygons_common.py for every forced index size; points all in one mixed cell and spread uniformly; one 1000-gon
under a 1 x 1 index (a list longer than any unroll, ragged against the loads in flight); hundreds of overlapping polygons (the
early exit) -- and pcr.points_in_polygons on a Device cloud and the HIP engine's polygon channels.  Everything BIT FOR BIT
against the host twin and the host engine, which tests/test_points_in_polygons.py holds to the brute-force model of the contract."""
import numpy as np
import pytest

import pcr
import points_in_polygons_common as PC
import reduction_filters_common as RF
import sample_grid_common as SG
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DEVICE = pcr.MemoryLocation.Device
PER_WG = 256 * 4                                                 # points per workgroup: 256 * PCR_HIP_POLYGON_POINTS_PER_LANE
COUNTS = [1, 63, 64, 65, 255, 256, 257, 2 * PER_WG + 37]
OFFSETS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]  # x, y, out: elements off 16 bytes


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def gpu_config(specs, cfg_filt=(), **kw):
    return RF.make_config("gpu", specs, cfg_filt, SG.PGRID, **kw)


def cpu_config(specs, cfg_filt=(), **kw):
    return RF.make_config("cpu", specs, cfg_filt, SG.PGRID, **kw)


_lattices = {}


def lattice_of(name):
    if name not in _lattices:
        polys = PC.SETS[name]()
        x, y = PC.lattice(polys, [s for s in PC.INDEX_SIZES if s != (0, 0)])
        _lattices[name] = (polys, x, y)
    return _lattices[name]


def test_counts_and_alignments(A):
    polys, x, y = lattice_of("partition")
    rng = np.random.default_rng(1)
    pick = rng.permutation(len(x))
    with PC.Index(A, polys, 7, 5) as ix:
        want = ix.host(x, y)
        assert (~np.isnan(want)).sum() > 100 and np.isnan(want).sum() > 100
        for n in COUNTS:
            sel = pick[:n]
            xs, ys = np.ascontiguousarray(x[sel]), np.ascontiguousarray(y[sel])
            for off in OFFSETS:
                PC.bits_equal(ix.device(xs, ys, *off), want[sel], f"n = {n}, offsets {off}")
        assert ix.L.pcr_hip_points_in_polygons(ix.ptr, ix.d_tables.ptr, None, None, 0, None, None, None) == 0      # n == 0


@pytest.mark.parametrize("name", sorted(PC.SETS))
def test_the_lattice_for_every_index_size(A, name):
    polys, x, y = lattice_of(name)
    first = None
    for cols, rows in PC.INDEX_SIZES:
        with PC.Index(A, polys, cols, rows) as ix:
            want = ix.host(x, y)
            PC.bits_equal(ix.device(x, y), want, f"{name}, index {cols} x {rows}")
            PC.bits_equal(ix.device(x, y, 1, 0, 1), want, f"{name}, index {cols} x {rows}, element-wide")
        first = want if first is None else first
        PC.bits_equal(want, first, f"{name}: index {cols} x {rows} against 1 x 1")


def test_one_mixed_cell_and_a_uniform_spread(A):
    """Every lane walks a list (all points in one cell that an edge of the donut crosses), and most lanes do not."""
    polys = PC.donut()
    rng = np.random.default_rng(5)
    n = 2 * PER_WG + 37
    with PC.Index(A, polys, 64, 64) as ix:
        v, ring = polys.coords, polys.polygon(0)[0]
        x0, y0 = v[:, 0].min(), v[:, 1].min()
        cw, ch = (v[:, 0].max() - x0) / 64, (v[:, 1].max() - y0) / 64
        mid = (ring[3] + ring[4]) / 2                              # the cell that holds the middle of an edge of the outer ring
        i, j = int((mid[0] - x0) / cw), int((mid[1] - y0) / ch)
        x, y = rng.uniform(x0 + (i + 0.02) * cw, x0 + (i + 0.98) * cw, n), rng.uniform(y0 + (j + 0.02) * ch, y0 + (j + 0.98) * ch, n)
        want = ix.host(x, y)
        assert 0 < (~np.isnan(want)).sum() < n, "the cell is mixed: points on both sides of the ring"
        PC.bits_equal(ix.device(x, y), want, "one mixed cell")
        x, y = rng.uniform(5.0, 55.0, 20000), rng.uniform(5.0, 55.0, 20000)
        want = ix.host(x, y)
        assert 2000 < (~np.isnan(want)).sum() < 18000
        PC.bits_equal(ix.device(x, y), want, "uniform spread")
        PC.bits_equal(want, PC.model(polys, x, y), "host twin against the model")


@pytest.mark.parametrize("edges", [1000, 1001, 1003])
def test_a_long_list_ragged_against_the_loads_in_flight(A, edges):
    polys = PC.big_ngon(edges)
    rng = np.random.default_rng(edges)
    x, y = rng.uniform(5.0, 95.0, 3000), rng.uniform(5.0, 95.0, 3000)
    lx, ly = PC.lattice(polys)
    x, y = np.concatenate([x, lx]), np.concatenate([y, ly])
    with PC.Index(A, polys, 1, 1) as ix:
        info = ix.info()
        assert (info["cols"], info["rows"], info["items"]) == (1, 1, 1) and info["listed_edges"] >= edges - 2
        want = ix.host(x, y)
        PC.bits_equal(ix.device(x, y), want, f"{edges}-gon, 1 x 1")
    with PC.Index(A, polys) as ix:
        PC.bits_equal(ix.device(x, y), want, f"{edges}-gon, automatic")


def test_long_lists_that_do_not_hold_the_point(A):
    """Overlapping polygons of many edges under coarse indexes: a point queued at one long list (more than 16 edges) that does
    not hold it walks on, as a wave, through further long lists, short ones and flagged cells; few points (the queue of 256
    takes them all) and many (it fills, and the rest walk alone)."""
    import rasterize_common as RC
    rng = np.random.default_rng(8)
    rings = [[RC.ngon(rng.uniform(30, 70), rng.uniform(30, 70), rng.uniform(15, 45), int(n), rng.uniform(0, 1))]
             for n in (17, 40, 64, 65, 100, 129, 33, 200)]
    rings += [[RC.ngon(rng.uniform(10, 90), rng.uniform(10, 90), rng.uniform(3, 12), int(rng.integers(3, 17)))] for _ in range(12)]
    polys = PC.Polys(rings)
    x, y = rng.uniform(-5.0, 105.0, 6000), rng.uniform(-5.0, 105.0, 6000)
    want = PC.model(polys, x, y)
    assert len(set(want[~np.isnan(want)].tolist())) >= 12 and np.isnan(want).sum() > 100
    for cols, rows in ((1, 1), (2, 3), (7, 5), (0, 0)):
        with PC.Index(A, polys, cols, rows) as ix:
            PC.bits_equal(ix.host(x, y), want, f"host twin, index {cols} x {rows}")
            PC.bits_equal(ix.device(x, y), want, f"6000 points, index {cols} x {rows}")
            PC.bits_equal(ix.device(x, y, 1, 1, 0), want, f"6000 points, element-wide, index {cols} x {rows}")
            for n in (1, 100, 255):
                PC.bits_equal(ix.device(x[:n].copy(), y[:n].copy()), want[:n], f"{n} points, index {cols} x {rows}")


def test_overlapping_polygons_the_early_exit(A):
    polys = PC.ngons()
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-80.0, 280.0, 30000), rng.uniform(-80.0, 230.0, 30000)
    payload = 0x7FC0BEEF
    for cols, rows in ((1, 1), (0, 0)):
        with PC.Index(A, polys, cols, rows, background_bits=payload) as ix:
            want = ix.host(x, y, threads=4)
            got = ix.device(x, y)
            PC.bits_equal(got, want, f"300 n-gons, index {cols} x {rows}")
            out = np.isnan(got)
            assert 100 < out.sum() < 29000 and (got.view(np.uint32)[out] == payload).all()


def test_points_in_polygons_on_a_device_cloud():
    polys, x, y = lattice_of("ngons")
    z = np.arange(len(x), dtype=F32)
    host = SG.make_cloud(pcr, x, y, {"z": z})
    dev = SG.make_cloud(pcr, x, y, {"z": z}, DEVICE)
    for kw in (dict(), dict(channel="plot", background=-1.0, index_cols=7, index_rows=5)):
        pcr.points_in_polygons(host, polys.to_pcr(), **kw)
        pcr.points_in_polygons(dev, polys.to_pcr(), **kw)
        name = kw.get("channel", "polygon")
        back = dev.to_host()
        PC.bits_equal(np.asarray(back.channel_array_f32(name)), np.asarray(host.channel_array_f32(name)), f"Device cloud, {kw}")
        assert (np.asarray(back.channel_array_f32("z")) == z).all()
    PC.bits_equal(np.asarray(host.channel_array_f32("polygon")), PC.model(polys, x, y), "Host cloud against the model")
    with pytest.raises(RuntimeError, match="index_cols and index_rows must be"):
        pcr.points_in_polygons(dev, polys.to_pcr(), index_cols=-1)


def test_hip_pipeline_clip_and_per_plot_counts():
    for location in (None, DEVICE):
        got = PC.check_clip_and_counts(pcr, gpu_config, location, what=f"HIP engine, {location}")
    want = PC.check_clip_and_counts(pcr, cpu_config, what="host engine")
    assert len(got) == len(want)
    for b, (u, w) in enumerate(zip(got, want)):
        SG.bits_equal(u, w, f"HIP engine against the host engine: band {b}")


def test_hip_pipeline_set_polygons_between_ingests():
    got = PC.check_set_polygons_again(pcr, gpu_config, DEVICE)
    want = PC.check_set_polygons_again(pcr, cpu_config)
    for b, (u, w) in enumerate(zip(got, want)):
        SG.bits_equal(u, w, f"HIP engine against the host engine: band {b}")


def test_hip_pipeline_histogram_file_and_reprojection(tmp_path):
    PC.check_histogram(pcr, gpu_config, DEVICE)
    PC.check_chunked_file(pcr, gpu_config, tmp_path)
    PC.check_reprojected(pcr, "gpu", DEVICE)


def test_hip_pipeline_refusals():
    PC.check_pipeline_refusals(pcr, "gpu", gpu_config)
