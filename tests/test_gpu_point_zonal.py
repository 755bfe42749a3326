"""Point zonal tables on the MI355X: pcr_hip_point_fold_stats and pcr_hip_point_fold_hist through the C-ABI -- paths 1, 2 and 0,
clouds of less than a wave up to several trips of every persistent workgroup, every way equal labels can lie in a wave, aligned
and misaligned inputs, no mask, seeded tables that wrap, tables and info words between sentinels, the capacity at which path 0
switches -- and the HIP engine's PipelineConfig.point_zonal.  Everything BIT FOR BIT against the host twins and the host engine,
which tests/test_point_zonal.py holds to the model of the contract."""
import ctypes as C

import numpy as np
import pytest

import pcr
import point_zonal_common as P
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32, U8, U64 = np.float32, np.uint8, np.uint64
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU
ZCAP = 9
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025]
PATHS = [1, 2, 0]
BINS = 64
HIST = (-3.0, BINS / 64.0)


@pytest.fixture(scope="module")
def A():
    return load_cabi()


@pytest.mark.parametrize("n", SIZES)
def test_kernels_equal_the_host_twins(A, n):
    values, mask = P.values_for(n), P.masks_for(n)
    for name, labels in P.label_patterns(n, ZCAP).items():
        want = P.run_fold_stats(A, False, labels, mask, values, ZCAP, seed=P.SEED, info=(2, P.SEED))
        want_h = P.run_fold_hist(A, False, labels, mask, values, ZCAP, BINS, *HIST, seed=P.SEED)
        for path in PATHS:
            what = f"n {n} {name} path {path}"
            P.same(P.run_fold_stats(A, True, labels, mask, values, ZCAP, path=path, seed=P.SEED, info=(2, P.SEED)), want, what)
            P.same(P.run_fold_hist(A, True, labels, mask, values, ZCAP, BINS, *HIST, path=path, seed=P.SEED), want_h, what + " hist")
    labels = P.label_patterns(n, ZCAP)["edge labels scattered in"]
    model = P.fold(labels, mask, values, ZCAP, stat=(0.0, 100.0))             # the model itself, info words included
    for path in (1, 2):
        P.same(P.run_fold_stats(A, True, labels, mask, values, ZCAP, path=path), model, f"n {n} path {path}: the model")
        only = P.run_fold_stats(A, True, labels, mask, None, ZCAP, path=path)
        P.same(only, dict(points=model["points"], info=model["info"]), f"n {n} path {path}: points alone")
        none = P.run_fold_stats(A, True, labels, None, values, ZCAP, path=path, points=False, info=None)
        P.same(none, P.run_fold_stats(A, False, labels, None, values, ZCAP, points=False, info=None), f"n {n} path {path}: no mask")


# Every persistent workgroup makes at least two trips, and the last tile is ragged: with `blocks` workgroups a trip of all of them
# reads blocks * BLOCK * POINTS_PER_LANE * TILES_IN_FLIGHT points (half of that on the element-wise variant, which then makes
# four).  The default launch has as many workgroups as trips up to 8 per CU -- two trips each would take 17 M points -- so the
# test asks for 16 workgroups: 2 * 16 * 4096 + 1024 + 77 = 132 173 points.
BLOCKS = 16


def two_trips(A):
    return 2 * BLOCKS * A.POINT_FOLD_BLOCK * A.POINT_FOLD_POINTS_PER_LANE * A.POINT_FOLD_TILES_IN_FLIGHT + \
        A.POINT_FOLD_BLOCK * A.POINT_FOLD_POINTS_PER_LANE + 77


@pytest.fixture(scope="module")
def big(A):
    n = two_trips(A)
    values, mask = P.values_for(n), P.masks_for(n)
    pats = P.label_patterns(n, ZCAP)
    across = np.full(n, 3.0, F32)
    across[1000:1100] = 6.0                  # one run across a wave's end (point 1023) and a workgroup's (tile 0 | tile 1)
    across[4090:4100] = 2.0                  # ... and across a trip's tiles
    cases = {"runs of 200": pats["runs of 200"], "shuffled": pats["shuffled"], "edge labels scattered in": pats["edge labels scattered in"],
             "a run across a wave and a workgroup": across}
    want = {k: (P.run_fold_stats(A, False, lab, mask, values, ZCAP, seed=P.SEED, info=(0, 1)),
                P.run_fold_hist(A, False, lab, mask, values, ZCAP, BINS, *HIST),
                P.run_fold_stats(A, False, lab, None, values, ZCAP)) for k, lab in cases.items()}
    return n, values, mask, cases, want


# byte offsets of label, mask and value from a 16-byte boundary: aligned; each one element, or one byte, off
OFFSETS = [(0, 0, 0), (4, 0, 0), (0, 1, 0), (0, 0, 4), (0, 4, 0)]


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("off", OFFSETS)
def test_two_trips_of_every_workgroup(A, big, path, off):
    n, values, mask, cases, want = big
    for name, labels in cases.items():
        what = f"{name} path {path} off {off}"
        P.same(P.run_fold_stats(A, True, labels, mask, values, ZCAP, path=path, blocks=BLOCKS, seed=P.SEED, info=(0, 1), off=off),
               want[name][0], what)
        P.same(P.run_fold_hist(A, True, labels, mask, values, ZCAP, BINS, *HIST, path=path, blocks=BLOCKS, off=off), want[name][1],
               what + " hist")
    P.same(P.run_fold_stats(A, True, cases["shuffled"], None, values, ZCAP, path=path, blocks=BLOCKS, off=off), want["shuffled"][2],
           f"no mask path {path} off {off}")
    P.same(P.run_fold_stats(A, True, cases["shuffled"], None, values, ZCAP, path=path, off=off, calls=3), want["shuffled"][2],
           f"the default launch in three calls, path {path} off {off}")


def test_an_lds_table_is_flushed_when_its_packed_counts_are_full(A):
    """Path 2 packs n with the sum in one LDS word and counts points and bins in 32 bits; a workgroup flushes after every 2^20
    points it has read.  ONE workgroup, every point in zone 1 with a value at the upper clamp (the greatest word a point can
    add), over more than one epoch."""
    n = (1 << 20) + 4096 + 5
    labels = np.ones(n, F32)
    values = np.full(n, np.inf, F32)
    values[::1000] = -np.inf
    want = P.run_fold_stats(A, False, labels, None, values, 3)
    assert int(want["n"][0]) == n and int(want["s2"][0]) == n * (P.Q ** 2)
    P.same(P.run_fold_stats(A, True, labels, None, values, 3, path=2, blocks=1), want, "one workgroup, two epochs")
    want_h = P.run_fold_hist(A, False, labels, None, values, 3, 4, 0.0, 1.0)
    P.same(P.run_fold_hist(A, True, labels, None, values, 3, 4, 0.0, 1.0, path=2, blocks=1), want_h, "hist, two epochs")


def plan(A, Z, bins, n, path):
    got = [C.c_int(0), C.c_int(0), C.c_size_t(0)]
    prm = A.PointFoldParams(path, 0)
    A.check(A.lib().pcr_hip_point_fold_plan(Z, bins, n, C.byref(prm), *[C.byref(g) for g in got]))
    return got[0].value, got[1].value, got[2].value


@pytest.mark.parametrize("bins", [0, 1, 64, 65, 256])
def test_both_sides_of_the_switch(A, bins):
    """The largest capacity path 2 takes and one above it: path 2 refuses the second, path 0 gives the twins' bits on both."""
    cap = A.POINT_FOLD_LDS_BYTES // (4 * bins if bins else A.POINT_FOLD_STATS_ROW_BYTES)
    n = 5000
    rng = np.random.default_rng(bins)
    labels = rng.integers(1, cap + 4, n).astype(F32)
    labels[:8] = [cap, cap + 1, cap, 1, cap + 1, cap - 1, cap + 2, cap]
    values, mask = P.values_for(n), P.masks_for(n)
    mask[:8] = 1
    for Z in (cap, cap + 1):
        assert plan(A, Z, bins, n, 0)[0] == (2 if Z == cap else 1)
        for path in (0, 1) + ((2,) if Z == cap else ()):
            if bins:
                want = P.run_fold_hist(A, False, labels, mask, values, Z, bins, -3.0, bins / 64.0)
                P.same(P.run_fold_hist(A, True, labels, mask, values, Z, bins, -3.0, bins / 64.0, path=path), want, f"Z {Z} path {path}")
            else:
                want = P.run_fold_stats(A, False, labels, mask, values, Z)
                P.same(P.run_fold_stats(A, True, labels, mask, values, Z, path=path), want, f"Z {Z} path {path}")
        assert want["info"][0] == Z and want["info"][1] > 0
    with pytest.raises(A.PcrHipError, match=f"path 2 holds at most {cap} zones"):
        plan(A, cap + 1, bins, n, 2)
    with pytest.raises(A.PcrHipError, match=f"path 2 holds at most {cap} zones"):
        if bins:
            P.run_fold_hist(A, True, labels, mask, values, cap + 1, bins, -3.0, bins / 64.0, path=2)
        else:
            P.run_fold_stats(A, True, labels, mask, values, cap + 1, path=2)
    assert plan(A, cap, bins, n, 2)[2] == cap * (4 * bins if bins else A.POINT_FOLD_STATS_ROW_BYTES)


# ---- the HIP engine's PipelineConfig.point_zonal -----------------------------------------------------------------------------------
LOCATIONS = [None, pcr.MemoryLocation.HostPinned, pcr.MemoryLocation.Device]


@pytest.fixture(scope="module")
def host_case():
    """The clouds of tests/test_point_zonal.py through the host engine: the plots' table under the pipeline filter and the specs'
    own, and the table by the cloud's own `cls` channel."""
    import points_in_polygons_common as PP
    import sample_grid_common as SG
    polys, c = PP.plots(), PP.plot_points(3000, 21)
    p = P.plot_pipeline(pcr, "cpu", P.CFG_FILT, stat_filt=P.STAT_FILT, hist_filt=P.HIST_FILT)
    p.set_polygons("plot", polys.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c))
    q = P.plot_pipeline(pcr, "cpu", label="cls", max_zones=8)
    q.set_polygons("plot", polys.to_pcr())
    q.ingest(SG.dict_cloud(pcr, c))
    assert len(p.point_zonal(0)["zone"]) == 14 and len(q.point_zonal(0)["zone"]) == 5
    return polys, c, (p.point_zonal(0), p.point_zonal_histogram(0, 0)), q.point_zonal(0)


@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_equals_the_host_engine(host_case, location, wait):
    import sample_grid_common as SG
    import zonal_common as ZC
    polys, c, (want, counts), want_cls = host_case
    p = P.plot_pipeline(pcr, "gpu", P.CFG_FILT, stat_filt=P.STAT_FILT, hist_filt=P.HIST_FILT)
    q = P.plot_pipeline(pcr, "gpu", label="cls", max_zones=8)
    p.set_polygons("plot", polys.to_pcr())
    q.set_polygons("plot", polys.to_pcr())
    assert all(len(v) == 0 for v in p.point_zonal(0).values())
    n, clouds = len(c["x"]), []
    for k in range(3):
        clouds.append(SG.dict_cloud(pcr, P.piece(c, n * k // 3, n * (k + 1) // 3), location))      # (kept alive until the tables are read)
        for pipe in (p, q):
            pipe.ingest(clouds[-1]) if wait else pipe.ingest_async(clouds[-1])
    ZC.same_table(p.point_zonal(0), want, f"{location} wait {wait}")                               # (waits for the stream itself)
    P.bits_equal(p.point_zonal_histogram(0, 0), counts, "point_zonal_histogram")
    ZC.same_table(q.point_zonal(0), want_cls, "the cloud's own channel as the label")
    p.finalize() if wait else p.finalize_async()
    ZC.same_table(p.point_zonal(0), want, "after finalize")
    p.synchronize()
    with pytest.raises(RuntimeError, match="no point_zonal entry 1"):
        p.point_zonal(1)


def test_chunked_las_file(tmp_path):
    """ingest_file of a small LAS tile in five chunks, the polygon channel as the label: the HIP engine decodes the records in HBM,
    the host engine reads them through the reader; `z` is decoded for the entry alone."""
    import points_in_polygons_common as PP
    import reduction_filters_common as RF
    import sample_grid_common as SG
    import zonal_common as ZC
    path, c = PP.las_tile(tmp_path)
    polys = PP.plots()
    labels = PP.model(polys, c["x"], c["y"])
    tables = []
    for mode in ("cpu", "gpu"):
        cfg = RF.make_config(mode, [RF.S("Count", ch="plot")], (), SG.PGRID, polygon_channels=[pcr.PolygonChannelConfig("plot")],
                             point_zonal=[P.entry(pcr)])
        p = pcr.Pipeline.create(cfg)
        assert p is not None and p.engine() == ("host" if mode == "cpu" else "hip"), pcr.pipeline_create_error()
        p.set_polygons("plot", polys.to_pcr())
        assert p.ingest_file(path, 700) == len(c["x"])
        tables.append((p.point_zonal(0), p.point_zonal_histogram(0, 0)))
    ZC.same_table(tables[1][0], tables[0][0], "chunked ingest_file")
    P.bits_equal(tables[1][1], tables[0][1], "chunked ingest_file: the counts")
    assert int(tables[1][0]["points"].sum()) == int((labels >= 1).sum()) > 1000


def test_the_free_function_on_a_device_cloud(host_case):
    import sample_grid_common as SG
    import zonal_common as ZC
    polys, c, _, _ = host_case
    e = P.entry(pcr)
    host = pcr.point_zonal(SG.dict_cloud(pcr, c), "cls", e.cell_stats, e.histograms, max_zones=8)
    dev = pcr.point_zonal(SG.dict_cloud(pcr, c, pcr.MemoryLocation.Device), "cls", e.cell_stats, e.histograms, max_zones=8)
    ZC.same_table(dev, host, "pcr.point_zonal")
    assert len(dev["zone"]) == 5 and int(dev["points"].sum()) == len(c["x"])
    with pytest.raises(RuntimeError, match="carry a zone above max_zones = 2"):
        pcr.point_zonal(SG.dict_cloud(pcr, c, pcr.MemoryLocation.Device), "cls", max_zones=2)


def test_a_budget_too_small_for_the_tables_refuses():
    import reduction_filters_common as RF
    import sample_grid_common as SG
    cfg = RF.make_config("gpu", [RF.S("Count", ch="z")], (), SG.PGRID, point_zonal=[P.entry(pcr, label="cls", max_zones=64)])
    # the grid's state is one plane and one band of 40 x 24 floats, 7 680 bytes; the entry's tables 16 + 64 * (8 + 24 + 8 * 16) bytes
    cfg.gpu_memory_budget = 12000
    assert pcr.Pipeline.create(cfg) is None
    assert "point_zonal tables need the state in HBM" in pcr.pipeline_create_error()
    cfg.point_zonal = []
    assert pcr.Pipeline.create(cfg) is not None                              # (the grid alone fits)
    cfg.point_zonal = [P.entry(pcr, label="cls", max_zones=64)]
    cfg.gpu_memory_budget = 0
    p = pcr.Pipeline.create(cfg)
    assert p is not None and not p.out_of_core(), pcr.pipeline_create_error()
