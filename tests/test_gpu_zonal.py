"""Zonal tables on the MI355X: pcr_hip_zone_max, _fold_stats, _fold_hist, _rows_stats and _rows_percentiles through the C-ABI --
bands of less than a wave, exactly one, more than one block, strided windows between sentinels, every way equal labels can lie in
a wave, labels the kernels must ignore, tables between sentinel words -- and the HIP engine's PipelineConfig.zonal.  Everything
BIT FOR BIT against the host twins and the host engine, which tests/test_zonal.py holds to the model of the contract."""
import numpy as np
import pytest

import pcr
import trees_common as T
import zonal_common as Z
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32, U64 = np.float32, np.uint64
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU
LOCATIONS = [pcr.MemoryLocation.Host, pcr.MemoryLocation.Device]
# (rows, cols): a lane, one short of a wave, a wave, one more, rows that end on and off a wave, more than one block
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 64), (3, 65), (2, 130), (33, 200)]


@pytest.fixture(scope="module")
def A():
    return load_cabi()


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_host_twins(A, shape):
    h, w = shape
    planes = Z.random_planes(h, w, 7)
    cube = Z.random_cube(5, h, w, 8)
    for name, (labels, zmax) in Z.label_patterns(h, w).items():
        want = Z.run_fold_stats(A, False, labels, planes, zmax)
        want_counts = Z.run_fold_hist(A, False, labels, cube, zmax)
        assert Z.run_zone_max(A, True, labels) == Z.run_zone_max(A, False, labels), name
        for stride, offset in ((w, 0), (w + 5, 0), (w, 3), (w + 5, 3)):
            assert Z.run_zone_max(A, True, labels, stride=stride, offset=offset) == Z.zone_max(labels), name
            for combine in (1, 0):
                what = f"{shape} {name} stride {stride} offset {offset} combine {combine}"
                got = Z.run_fold_stats(A, True, labels, planes, zmax, combine=combine, stride=stride, offset=offset)
                for k in ("cells", "n", "s1", "s2"):
                    Z.bits_equal(got[k], want[k], f"{what}: {k}")
                Z.bits_equal(Z.run_fold_hist(A, True, labels, cube, zmax, combine=combine, stride=stride, offset=offset, gap=offset),
                             want_counts, what)
        only = Z.run_fold_stats(A, True, labels, None, zmax)
        assert list(only) == ["cells"]
        Z.bits_equal(only["cells"], want["cells"], f"{shape} {name}: cells alone")
        none = Z.run_fold_stats(A, True, labels, planes, zmax, cells=False)
        Z.bits_equal(none["s2"], want["s2"], f"{shape} {name}: no cells")


@pytest.mark.parametrize("combine", [1, 0])
def test_sums_that_carry(A, combine):
    labels, planes, zmax = Z.carry_planes()
    want = Z.run_fold_stats(A, False, labels, planes, zmax)
    assert int(want["n"][0]) > 2 ** 32
    got = Z.run_fold_stats(A, True, labels, planes, zmax, combine=combine)
    for k in want:
        Z.bits_equal(got[k], want[k], k)
    import cell_stats_common as K
    n, s1, s2 = (a.reshape(-1) for a in K.preset_states())
    n64 = n.astype(U64)
    n64[5] = (1 << 40) + 3
    for zn, zs1, zs2 in ((got["n"], got["s1"], got["s2"]), (n64, s1, s2)):
        for ddof in (0, 1):
            for origin, res in ((0.0, 0.01), (-2.0, 2.0 ** -6)):
                rows = Z.run_rows_stats(A, True, zn, zs1, zs2, origin, res, ddof)
                for name, g, m in zip(("mean", "var", "std"), rows, Z.run_rows_stats(A, False, zn, zs1, zs2, origin, res, ddof)):
                    Z.bits_equal(g, m, f"ddof {ddof} res {res}: {name}")


@pytest.mark.parametrize("bins", [1, 32, 256])
def test_histogram_bins(A, bins):
    qs = [0.0, 0.25, 0.5, 0.95, 1.0]
    lo, w = Z.hist_consts(-3.0, 61.0, bins)
    for h, wd in ((3, 65), (2, 130)):
        labels, zmax = Z.label_patterns(h, wd)["invalid labels scattered in"]
        cube = Z.random_cube(bins, h, wd, bins)
        want = Z.run_fold_hist(A, False, labels, cube, zmax + 1)
        for combine in (1, 0):
            Z.bits_equal(Z.run_fold_hist(A, True, labels, cube, zmax + 1, combine=combine, stride=wd + 5, offset=3, gap=2), want,
                         f"bins {bins} combine {combine}")
        got_n, got = Z.run_rows_percentiles(A, True, want, lo, w, qs)
        want_n, cols = Z.run_rows_percentiles(A, False, want, lo, w, qs)
        Z.bits_equal(got_n, want_n, "hist_n")
        for q, g, m in zip(qs, got, cols):
            Z.bits_equal(g, m, f"bins {bins} q {q}")
        only_n, _ = Z.run_rows_percentiles(A, True, want, lo, w, [])
        Z.bits_equal(only_n, want_n, "hist_n alone")
    labels, cube, zmax = Z.carry_cube(bins)                                # a rank in a bin of more than 2^32 points
    want = Z.run_fold_hist(A, False, labels, cube, zmax)
    assert int(want[0, bins - 1]) > 2 ** 32
    for combine in (1, 0):
        Z.bits_equal(Z.run_fold_hist(A, True, labels, cube, zmax, combine=combine), want, f"carry, combine {combine}")
    lo, w = Z.hist_consts(0.0, 64.0, bins)
    got_n, got = Z.run_rows_percentiles(A, True, want, lo, w, qs)
    want_n, cols = Z.run_rows_percentiles(A, False, want, lo, w, qs)
    Z.bits_equal(got_n, want_n, "carry: hist_n")
    for q, g, m in zip(qs, got, cols):
        Z.bits_equal(g, m, f"carry: q {q}")


# ---- the HIP engine's PipelineConfig.zonal -----------------------------------------------------------------------------------------
WP, HP = 130, 70


@pytest.fixture(scope="module")
def host_case():
    host = Z.create(pcr, Z.pipeline_cfg(pcr, WP, HP, CPU), "host")
    want = []
    for seed in (1, 2):
        host.ingest(Z.canopy_points(pcr, WP, HP, seed))
        host.finalize()
        want.append((host.zonal(0), host.zonal_histogram(0, 0), host.trees(0)))
    assert len(want[0][0]["zone"]) >= 50 and len(want[1][0]["zone"]) >= 50
    return want


@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_equals_the_host_engine(host_case, location, wait):
    pipe = Z.create(pcr, Z.pipeline_cfg(pcr, WP, HP, GPU, location), "hip")
    with pytest.raises(RuntimeError, match="no zonal entry 0"):
        pipe.zonal(0)
    for k, seed in enumerate((1, 2)):
        pipe.ingest(Z.canopy_points(pcr, WP, HP, seed))
        with pytest.raises(RuntimeError, match="no zonal entry 0"):
            pipe.zonal(0)
        if wait:
            pipe.finalize()
        else:
            pipe.finalize_async()                                         # (zonal() is enqueued behind it and waits itself)
        got, counts = pipe.zonal(0), pipe.zonal_histogram(0, 0)
        Z.same_table(got, host_case[k][0], f"finalize {k + 1}")
        Z.bits_equal(counts, host_case[k][1], f"finalize {k + 1}: zonal_histogram")
        assert got["cells"].tolist() == pipe.trees(0)["crown_cells"].tolist() == host_case[k][2]["crown_cells"].tolist()
        pipe.synchronize()
    with pytest.raises(RuntimeError, match="no zonal entry 1"):
        pipe.zonal(1)


@pytest.mark.parametrize("grid_location", LOCATIONS)
def test_external_zones(grid_location):
    plots = Z.plot_labels(WP, HP)
    tables = []
    for mode, engine in ((CPU, "host"), (GPU, "hip")):
        cfg = Z.pipeline_cfg(pcr, WP, HP, mode)
        cfg.zonal = [pcr.ZonalConfig("plots", external=True, cell_stats=[0], histograms=[0], percentiles=[0.1, 0.9]),
                     pcr.ZonalConfig("value_5", histograms=[0], max_zones=3)]
        pipe = Z.create(pcr, cfg, engine)
        pipe.ingest(Z.canopy_points(pcr, WP, HP, 1))
        pipe.finalize()
        with pytest.raises(RuntimeError, match="the label grid 'plots' was not set"):
            pipe.zonal(0)
        grid = T.make_grid([np.zeros_like(plots), plots])
        with pytest.raises(RuntimeError, match="set_zones: the grid is"):
            pipe.set_zones("plots", T.make_grid([plots[:-1]]))
        pipe.set_zones("plots", grid.to(grid_location), 1)
        del grid                                                          # (the pipeline keeps a copy of its own)
        tables.append((pipe.zonal(0), pipe.zonal_histogram(0, 0)))
        with pytest.raises(RuntimeError, match="is above max_zones = 3"):
            pipe.zonal(1)
    Z.same_table(tables[1][0], tables[0][0], "plots")
    Z.bits_equal(tables[1][1], tables[0][1], "plots: zonal_histogram")
    assert len(tables[0][0]["zone"]) == Z.zone_max(plots) == 45


def test_a_budget_too_small_refuses():
    cfg = Z.pipeline_cfg(pcr, WP, HP, GPU)
    cfg.trees, cfg.cell_stats, cfg.histograms = [], [], []
    cfg.zonal = [pcr.ZonalConfig("plots", external=True)]
    cfg.gpu_memory_budget = 2 * WP * HP * 4                              # not even the planes fit: the pipeline would run out of core
    assert pcr.Pipeline.create(cfg) is None
    assert "zonal tables need the state in HBM" in pcr.pipeline_create_error()
    cfg.gpu_memory_budget = 0
    pipe = Z.create(pcr, cfg, "hip")
    assert not pipe.out_of_core()
