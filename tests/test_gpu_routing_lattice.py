"""Points on cell edges (tests/routing_lattice.py) through every device kernel that decides where a point belongs.

world_to_cell on the device (csrc/common.hpp) multiplies by 1 / cell_size and falls back to the reference's true division
only when the product lands within a few ulps of an integer.  That fallback alone keeps such a point in the reference's cell,
reference tile, LDS tile, row band and rank -- and a uniform random cloud never reaches it.  The clouds here put hundreds of
points where the two formulas floor differently (tests/test_routing_lattice.py counts them), and run them through: the direct
and the binned Point scatter (one reference tile and many), the two-level sort and the row bands, a second ingest,
MostRecent, two row-block shards and pcr_hip_route_count, and the glyph paths, whose footprint is placed by the PRODUCT (as
the reference places it, glyph_kernels.cu:97-98) inside the tile of the DIVIDED cell.

Values are 1 + i % 7: Sum, Count, Max, Min and Average of a cell are exact in f32 whatever the order, so every Point band is
compared bit for bit.  Glyph bands are compared as tests/test_gpu_cabi_parity.py::test_glyph_cases_full_grid compares them."""
import ctypes as C
import functools

import numpy as np
import pytest

import pcr_oracle_py as O
from conftest import assert_band_close, load_cabi

import most_recent_common as M
import routing_lattice as R
from test_gpu_cabi_parity import RT, assert_glyph_close, cabi_grid
from test_gpu_most_recent import SelectRun

pytestmark = pytest.mark.gpu

POINT_BANDS = ["Sum", "Count", "Max", "Min", "Average"]


@pytest.fixture(scope="module")
def A():
    mod = load_cabi()
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@functools.lru_cache(maxsize=None)
def point_bands(name):
    """The oracle's five Point bands and its count of valid points: computed once per geometry."""
    og = R.grid(name)
    x, y, v = R.cloud(name)
    ref = O.Reduction(og, O.COUNT)
    ref.ingest(x, y, v)
    return {k: O.run(og, RT[k], x, y, v) for k in POINT_BANDS}, ref.points_valid()


def assert_point_bands(run, name, what):
    want, _ = point_bands(name)
    for k in POINT_BANDS:
        assert_band_close(run.finalize(RT[k]), want[k], what=f"{name}/{k} {what}")


@pytest.mark.parametrize("path", [1, 2, 0])
@pytest.mark.parametrize("name", R.NAMES)
def test_point_all_planes_in_one_scatter(A, name, path):
    """Plane mask 15: the direct kernels, and both ONE_TILE variants of k_bin_count (tenth_one_tile against the rest)."""
    x, y, v = R.cloud(name)
    run = A.ReductionRun(cabi_grid(A, R.grid(name)), 15, path=path)
    try:
        run.scatter(x, y, v)
        st = run.stats()
        assert path == 0 or st.path == path - 1
        assert st.points_in == len(x) and st.points_valid == point_bands(name)[1]
        assert_point_bands(run, name, f"path {path}")
    finally:
        run.close()


@pytest.mark.parametrize("mode", ["two_level", "bands"])
@pytest.mark.parametrize("name", R.HARD)
def test_point_two_level_sort_and_row_bands(A, monkeypatch, name, mode):
    """More LDS tiles than one binning pass may count: the two-level sort (the MULTI count variant), or row bands, where
    band_grid narrows the owned rows and a row decision sits on every band edge."""
    monkeypatch.setenv("PCR_HIP_DEBUG_MAX_BINS", "12")          # read by pcr_hip_engine_create
    monkeypatch.setenv("PCR_HIP_DEBUG_TWO_LEVEL", "1" if mode == "two_level" else "0")
    x, y, v = R.cloud(name)
    run = A.ReductionRun(cabi_grid(A, R.grid(name)), 15, path=2)
    try:
        run.scatter(x, y, v)
        st = run.stats()
        assert st.path == 1 and st.num_bins > 12, "the large-grid sweep was not taken"
        assert st.points_valid == point_bands(name)[1]
        assert_point_bands(run, name, mode)
    finally:
        run.close()


@pytest.mark.parametrize("path", [1, 2])
def test_second_ingest_of_the_same_cloud(A, path):
    """The first scatter defines undefined planes (planes_fresh = 2), the second accumulates on them (0): Sum and Count
    double, Max and Min stay."""
    name = "tenth"
    x, y, v = R.cloud(name)
    want, valid = point_bands(name)
    L = A.lib()
    run = A.ReductionRun(cabi_grid(A, R.grid(name)), 15, path=path)
    try:
        for b in run.bufs.values():
            A.check(L.pcr_hip_memset(b.ptr, 0xA5, b.nbytes, None))
        A.check(L.pcr_hip_engine_planes_fresh(run.engine, 2))
        run.scatter(x, y, v)
        assert run.stats().path == path - 1 and run.stats().points_valid == valid
        assert_point_bands(run, name, f"first ingest, path {path}")
        run.scatter(x, y, v)
        assert run.stats().points_valid == valid
        for k in ("Sum", "Count"):
            assert_band_close(run.finalize(RT[k]), 2.0 * want[k], what=f"{k} after the second ingest")
        for k in ("Max", "Min", "Average"):
            assert_band_close(run.finalize(RT[k]), want[k], what=f"{k} after the second ingest")
    finally:
        run.close()


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("name", R.HARD)
def test_most_recent(A, name, path):
    """pcr_hip_scatter_select with all-distinct timestamps: the state words and the band, against the literal loop of the
    reference's combine_timestamped over the oracle's cells."""
    og = R.grid(name)
    x, y, v = R.cloud(name)
    t = np.arange(len(x), dtype=np.float32)                    # distinct, below 2^24
    cell = M.cells_oracle(og, x, y)
    shape = (og.height, og.width)
    run = SelectRun(A, cabi_grid(A, og), path)
    try:
        run.scatter(x, y, v, t)
        st = run.stats()
        assert st.path == path - 1 and st.points_valid == int((cell >= 0).sum())
        assert np.array_equal(run.words(), M.fold_words(cell, v, t, shape[0] * shape[1])), "state words"
        M.assert_bits(run.finalize(), M.reference_loop(cell, v, t, shape, range(len(x))), f"{name}, path {path}")
    finally:
        run.close()


def split_row(og, x, y):
    """The row whose upper edge most disagreeing y values sit on: one formula says this row, the other the row above."""
    div, mul = R.quotients(og, x, y)
    edge = np.maximum(div[1], mul[1])[R.disagreements(og, x, y)[1]].astype(np.int64)
    edge = edge[(edge > 0) & (edge < og.height)]
    assert len(edge) > 0
    return int(np.bincount(edge).argmax())


@pytest.mark.parametrize("halo", [0, 4])
@pytest.mark.parametrize("path", [1, 2])
def test_two_row_blocks_take_every_point_exactly_once(A, path, halo):
    name = "tenth"
    og = R.grid(name)
    x, y, v = R.cloud(name)
    want, valid = point_bands(name)
    k = split_row(og, x, y)
    got, seen = [], 0
    for own in ((0, k), (k, og.height)):
        run = A.ReductionRun(cabi_grid(A, og, own_rows=own, halo=halo), A.PLANE_WGT, path=path)
        try:
            run.scatter(x, y, v)                                # every shard sees the whole cloud and keeps its own rows
            seen += run.stats().points_valid
            got.append(run.finalize(RT["Count"]))
        finally:
            run.close()
    assert_band_close(np.vstack(got), want["Count"], what=f"rows split at {k}, halo {halo}, path {path}")
    assert seen == valid


@pytest.mark.parametrize("name", R.HARD)
def test_route_count_gives_every_point_its_owner(A, name):
    og = R.grid(name)
    x, y, _ = R.cloud(name)
    k = split_row(og, x, y)
    _, row, ok = R.cells(og, x, y)
    want = np.where(ok, (row >= k).astype(np.uint8), np.uint8(255)).astype(np.uint8)
    on_edge = R.disagreements(og, x, y)[1] & ((row == k) | (row == k - 1))
    assert on_edge.sum() >= 1                                    # the split is a row edge the two formulas disagree on
    L = A.lib()
    n = len(x)
    g = cabi_grid(A, og)
    dx, dy = A.DeviceBuffer.from_numpy(np.array(x)), A.DeviceBuffer.from_numpy(np.array(y))
    ddest, dcount = A.DeviceBuffer(n), A.DeviceBuffer(8 * 2)
    splits = (C.c_int32 * 3)(0, k, og.height)
    A.check(L.pcr_hip_route_count(C.byref(g), splits, 2, dx.ptr, dy.ptr, None, n, ddest.ptr, dcount.ptr, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    dest = ddest.to_numpy(np.uint8, (n,))
    bad = np.nonzero(dest != want)[0]
    assert len(bad) == 0, f"{len(bad)} points with the wrong owner, first ({x[bad[0]]!r}, {y[bad[0]]!r})"
    assert dcount.to_numpy(np.uint64, (2,)).tolist() == [int((want == p).sum()) for p in range(2)]


# sigma and half length in world units (cell size 0.1).  On these clouds the f32 oracle and the wide oracle have the same
# NaN mask (no cell excused by the 1e-6 cut-off rule), so the sigmas stand as the round numbers they are.
GLYPHS = {
    "gauss_cells_r3": dict(type=O.GLYPH_GAUSSIAN, sigma_x=0.1, sigma_y=0.1, max_radius=3.0),      # cell tiles, classify<CENTRE>
    "gauss_index_r5": dict(type=O.GLYPH_GAUSSIAN, sigma_x=0.15, sigma_y=0.15, max_radius=6.0),    # Index records
    "gauss_moments_r12": dict(type=O.GLYPH_GAUSSIAN, sigma_x=0.4, sigma_y=0.4, max_radius=12.0),  # path 3: moments
    "line": dict(type=O.GLYPH_LINE, direction=0.6, half_length=0.35, max_radius=32.0),
}
GLYPH_RUNS = [(s, p) for s in GLYPHS for p in ((3, 1, 2, 0) if s == "gauss_moments_r12" else (1, 2, 0))]


@functools.lru_cache(maxsize=None)
def glyph_bands(name, spec, rname):
    og = R.grid(name)
    x, y, v = R.cloud(name)
    gl = O.make_glyph(**GLYPHS[spec])
    ref = O.Reduction(og, RT[rname], gl)
    ref.ingest(x, y, v)
    exact = O.run(og, RT[rname], x, y, v, glyph=gl, wide=True).astype(np.float64)
    return ref.finalize(), exact, ref.points_valid()


@pytest.mark.parametrize("rname", ["Count", "WeightedAverage"])
@pytest.mark.parametrize("spec,path", GLYPH_RUNS, ids=[f"{s}-path{p}" for s, p in GLYPH_RUNS])
@pytest.mark.parametrize("name", ["tenth", "tenth_one_tile"])
def test_glyphs(A, name, spec, path, rname):
    """Reference tiles of 16 x 16 (the clip matters) and one tile.  Where the product and the division floor differently the
    footprint's centre lies one cell outside the tile the point was routed to."""
    x, y, v = R.cloud(name)
    want, exact, valid = glyph_bands(name, spec, rname)
    mask = A.PLANE_WGT if rname == "Count" else A.PLANE_SUM | A.PLANE_WGT
    run = A.ReductionRun(cabi_grid(A, R.grid(name)), mask, path=path)
    try:
        run.scatter(x, y, v, glyph=GLYPHS[spec])
        st = run.stats()
        got = run.finalize(RT[rname])
    finally:
        run.close()
    assert path == 0 or st.path == {1: 0, 2: 1, 3: 2}[path]
    assert st.points_valid == valid
    is_line = GLYPHS[spec]["type"] == O.GLYPH_LINE
    assert_glyph_close(got, want, exact, f"{name}/{spec}/{rname} path {path}", is_line)
    # cells excused by the 1e-6 cut-off rule: at most 0.1 % of the touched cells
    assert (np.isnan(got) != np.isnan(want)).sum() <= 1e-3 * (~np.isnan(want)).sum()
