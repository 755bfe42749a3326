"""Gaussian splats of radius above 20 cells through the splat kernels (k_gauss_direct, k_tile_gauss; glyph_device.hpp):
this file owns those radii -- test_gpu_fuzz.py and the golden cases stop at 20, test_gpu_moments.py covers larger
ones on the moment path only, which per-point sigma / rotation channels and a non-zero default rotation never take.

Covered here, each test asserting from a restatement of the geometry (gauss_large_radius_common.py) and from the
engine's stats that the branch it is named for was taken:
  1. isolated footprints: the narrow form with one row per step, the wide form with two and three column blocks and
     a ragged last block, the row table refreshed per 64 rows, windows clipped at reference-tile and grid edges;
  2. the generic loop: rotated, wider than 192 columns, and windows on both sides of 2^18 cells;
  3. dense overlap with max_radius on both sides of what the LDS apron covers (the global-atomic spill of finite weights);
  4. the tile side grown at the apron's expense under a small bin limit, swept in row bands;
  5. row-block shards with a halo taller than the apron;
  6. non-finite rotation / sigma channels at radius 40;
  7. the same through pcr.Pipeline on the Auto path;
  8. a seeded fuzz over the large-radius space, compared as test_gpu_fuzz.py compares its own cases.
Reference: the CPU oracle accumulated in binary64; the float32 oracle where a mask is compared.
Bars: isolated footprints with a dead cut-off -- the set of cells exact, every cell within 1e-5 relative (both sides evaluate
the same float32 expression; |argument of expf| <= 13.8 where w >= 1e-6, so a few ulp of difference in the argument is below
6e-6 relative in w, two expf implementations add < 3e-7).  Everything else: the project's glyph bar, rtol 1e-4 with a floor of
1e-3 of the value scale, mask flips on the 1e-6 cut-off at most max(2, 1e-4 * cells)."""
import math

import numpy as np
import pytest

import pcr_oracle_py as O
import gauss_large_radius_common as G
from conftest import load_cabi
from test_gpu_cabi_parity import assert_glyph_close, gpu_run
from test_gpu_fuzz import _glyph_shards_add_up, check_case_matches_oracle
from test_gpu_moments import check
from test_gpu_row_bands import few_bins  # noqa: F401  (fixture: PCR_HIP_DEBUG_MAX_BINS=6)

pytestmark = pytest.mark.gpu
RT = G.RT
GAUSS = O.GLYPH_GAUSSIAN


@pytest.fixture(scope="module")
def A():
    return load_cabi()


def glyphs(A, sigma=(1.0, 1.0), rotation=0.0, max_radius=32.0):
    gl = dict(type=A.GLYPH_GAUSSIAN, sigma_x=sigma[0], sigma_y=sigma[1], rotation=rotation, max_radius=max_radius)
    return gl, O.make_glyph(GAUSS, sigma_x=sigma[0], sigma_y=sigma[1], rotation=rotation, max_radius=max_radius)


def assert_path(st, path, mask, max_radius, covered=None):
    """path 1: the direct kernel ran; path 2: the LDS tiles ran with the tile and apron glyph_tile derives from the reach."""
    if path == 1:
        assert st.path == 0, "the direct path was not taken"
        return
    need = math.ceil(max_radius)
    S, apron = G.lds_geometry(mask, need)
    assert st.path == 1 and (st.lds_tile_w, st.lds_tile_h, st.lds_apron) == (S, S, apron), \
        (st.path, st.lds_tile_w, st.lds_apron, S, apron)
    if covered is not None:
        assert (st.lds_apron >= need) == covered and (st.lds_apron < need) == (not covered)


def assert_isolated_exact(got, want32, exact, what):
    """One weight per cell and a dead cut-off: no allowance.  Cells exact, values 1e-5 relative to the binary64 oracle."""
    gm, wm, em = G.contributed(got), G.contributed(want32), G.contributed(exact)
    assert np.array_equal(wm, em), f"{what}: the two oracles disagree on the cells"
    assert np.array_equal(np.isnan(got), np.isnan(exact)), f"{what}: NaN mask"
    assert np.array_equal(gm, em), f"{what}: {int((gm & ~em).sum())} extra, {int((em & ~gm).sum())} missing cells"
    rel = np.abs(got[em].astype(np.float64) - exact[em].astype(np.float64)) / np.abs(exact[em].astype(np.float64))
    print(f"{what}: max rel err {rel.max():.3e} over {int(em.sum())} cells")
    assert rel.max() <= 1e-5, f"{what}: max rel err {rel.max():.3e}"


def run_isolated(A, og, cl, ch, rot, maxr, path, exact_bar, what, n_cells=None):
    """Count of unit values (every cell holds exactly one weight), Sum of distinct values, WeightedAverage."""
    gl, ogl = glyphs(A, rotation=rot, max_radius=maxr)
    for rname in ("Count", "Sum", "WeightedAverage"):
        v = np.ones(len(cl["x"]), np.float32) if rname == "Count" else cl["v"]
        got, st = gpu_run(A, og, RT[rname], [dict(x=cl["x"], y=cl["y"], value=v, **ch)], glyph=gl, path=path)
        assert_path(st, path, G.PLANE_MASK[rname], maxr)
        assert st.points_valid == len(v)
        want = O.run(og, RT[rname], cl["x"], cl["y"], v, glyph=ogl, **ch)
        exact = O.run(og, RT[rname], cl["x"], cl["y"], v, glyph=ogl, wide=True, **ch)
        tag = f"{what}/{rname}/path {path}"
        if exact_bar:
            if rname == "Count":
                assert np.nanmin(exact) > 2e-6, "the 1e-6 cut-off is not dead on these inputs"
                assert int(G.contributed(exact).sum()) == n_cells
            assert_isolated_exact(got, want, exact, tag)
        else:
            assert np.array_equal(np.isnan(want), np.isnan(exact)), f"{tag}: the two oracles disagree on the mask"
            assert_glyph_close(got, want, exact.astype(np.float64), tag, False)
            if rname != "WeightedAverage":                           # nothing painted where the oracle painted nothing
                assert np.abs(got[~G.contributed(exact) & ~np.isnan(got)]).max(initial=0.0) <= 2e-6 * float(v.max())


# ---- 1. isolated footprints ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", G.part1_cases(), ids=lambda c: c[0])
def test_isolated_footprints_every_form_of_the_wave_splat(A, case, path):
    name, grid, pts = case
    og = O.make_grid(grid["bounds"], tile=grid["tile"])
    wins = [G.window(og, *p) for p in pts]
    forms = {(G.branch(w, h, True), h > 64) for _, _, w, h, _ in wins}
    if name == "unclipped":
        assert [(w, h) for _, _, w, h, _ in wins] == [(2 * p[2] + 1,) * 2 for p in pts] and {p[2] for p in pts} == set(G.RADII)
        # r 21..31: narrow, one row per step; 32..95: two and three column blocks, ragged; 96 and up: the generic loop
        assert forms == {("narrow", False), ("wide", True), ("generic", True)}
    else:
        assert any(cut for *_, cut in wins) or any(w == 1 or h == 1 for _, _, w, h, _ in wins)
        assert forms & {("narrow", True), ("wide", True), ("wide", False), ("narrow", False)}
    cl = G.isolated_cloud(og, pts)
    ch = dict(sigma_x=cl["sigma_x"], sigma_y=cl["sigma_y"])
    run_isolated(A, og, cl, ch, 0.0, 130.0, path, True, name, n_cells=sum(w * h for _, _, w, h, _ in wins))


def test_isolated_layouts_cover_the_named_window_shapes():
    """The clipped (wdt, hgt) pairs the layouts above produce, computed here: every width and height at which the wave
    splat changes its form or its block count, wide-and-short and narrow-and-tall among them."""
    pairs = set()
    for name, grid, pts in G.part1_cases()[1:]:
        og = O.make_grid(grid["bounds"], tile=grid["tile"])
        pairs |= {G.window(og, *p)[2:4] for p in pts}
    assert {w for w, _ in pairs} >= set(G.WDT_SET) and {h for _, h in pairs} >= set(G.HGT_SET)
    assert any(w >= 3 * h and w > 64 for w, h in pairs) and any(h >= 3 * w and h > 64 for w, h in pairs)


# ---- 2. the generic loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", G.PART2_CASES, ids=lambda c: c["name"])
def test_generic_loop_rotated_wide_and_large_windows(A, case, path):
    og = O.make_grid(G.GRID_GENERIC, tile=case["tile"])
    rotated = G.case_is_rotated(case)
    wins = [G.window(og, *p[:3]) for p in case["pts"]]
    assert {G.branch(w, h, not rotated) for _, _, w, h, _ in wins} == case["want"]
    if "dims" in case:
        assert [(w, h) for _, _, w, h, _ in wins] == [case["dims"]]
        assert (case["dims"][0] * case["dims"][1] >= 1 << 18) == (case["want"] == {"generic-div"})
    cl = G.isolated_cloud(og, case["pts"])
    ch = dict(sigma_x=cl["sigma_x"], sigma_y=cl["sigma_y"])
    if case["rot_chan"]:
        ch["rotation"] = cl["rotation"]
    run_isolated(A, og, cl, ch, case["def_rot"], case["maxr"], path, not rotated, case["name"],
                 n_cells=sum(w * h for _, _, w, h, _ in wins))


# ---- 3. dense overlap through the spill -----------------------------------------------------------------------------------------
_dense_ref = {}


def dense_reference(og, key, rname, maxr):
    """The two oracle bands of a dense case, computed once and shared by the paths."""
    if key not in _dense_ref:
        cl = G.dense_cloud(og, rname)
        ogl = O.make_glyph(GAUSS, sigma_x=G.DENSE_SIGMA_Y * og.cell_size_x, sigma_y=G.DENSE_SIGMA_Y * abs(og.cell_size_y), max_radius=maxr)
        want = O.run(og, RT[rname], cl["x"], cl["y"], cl["value"], glyph=ogl, sigma_x=cl["sigma_x"])
        exact = O.run(og, RT[rname], cl["x"], cl["y"], cl["value"], glyph=ogl, wide=True, sigma_x=cl["sigma_x"])
        assert np.array_equal(np.isnan(want), np.isnan(exact)), "the two oracles disagree on the mask"
        want.setflags(write=False)
        exact.setflags(write=False)
        _dense_ref[key] = (want, exact)
    return _dense_ref[key]


def run_dense(A, og, key, rname, maxr, covered, path, what):
    cl = G.dense_cloud(og, rname)
    gl, _ = glyphs(A, sigma=(G.DENSE_SIGMA_Y * og.cell_size_x, G.DENSE_SIGMA_Y * abs(og.cell_size_y)), max_radius=maxr)
    got, st = gpu_run(A, og, RT[rname], [cl], glyph=gl, path=path)
    assert_path(st, path, G.PLANE_MASK[rname], maxr, covered)
    want, exact = dense_reference(og, key, rname, maxr)
    # reaches beyond the apron are really there: per-point sigmas up to 22 cells, capped by max_radius
    assert G.radius_cells(22.0, maxr) == min(66, math.ceil(maxr))
    if rname == "Sum":
        check(got, want, exact.astype(np.float64), what, scale=10.0)
    else:
        assert_glyph_close(got, want, exact.astype(np.float64), what, False)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("tile", [(4096, 4096), (200, 128)], ids=["one-tile", "tiles-200x128"])
@pytest.mark.parametrize("maxr,rname,covered", G.DENSE_CASES, ids=lambda v: str(v))
def test_dense_overlap_at_the_edges_of_the_apron(A, maxr, rname, covered, tile, path):
    og = G.dense_grid(tile)
    run_dense(A, og, (tile, maxr, rname), rname, maxr, covered, path, f"dense r<={maxr} {rname} tile {tile} path {path}")


@pytest.mark.parametrize("path", [1, 2])
def test_dense_overlap_unequal_cells_and_offset_origin(A, path):
    og = G.dense_grid((200, 128), cell=(0.5, -2.5), origin=(1000.5, -200.25))
    for rname in ("WeightedAverage", "Sum"):
        run_dense(A, og, ("cells", 64.0, rname), rname, 64.0, False, path, f"dense cell (0.5, -2.5) {rname} path {path}")


def test_dense_blob_split_into_several_work_items(A):
    """2400 of 3000 points in one 32 x 32 LDS tile at a reach of 33: the bin is split into three work items of 1024 points,
    whose windows are merged with atomics and whose spills meet in the same cells."""
    W, H = G.DENSE_GRID
    og, maxr, S = G.dense_grid((4096, 4096)), 33.0, 32
    rng = np.random.default_rng(37)
    n, k = 3000, 2400
    fx, fy = rng.uniform(-3.0, W + 3.0, n), rng.uniform(-3.0, H + 3.0, n)
    fx[:k], fy[:k] = rng.normal(5 * S + 16.0, 4.0, k), rng.normal(3 * S + 16.0, 4.0, k)
    x, y = og.min_x + fx, og.max_y - fy
    v = rng.uniform(5.0, 15.0, n).astype(np.float32)
    sx = rng.uniform(8.0, 22.0, n).astype(np.float32)
    assert G.lds_geometry(3, 33) == (S, 32) and G.item_points(33) == 1024
    in_bin = (np.floor(fx) // S == 5) & (np.floor(fy) // S == 3)
    assert in_bin.sum() > 2 * G.item_points(33), "the blob's bin is not split"
    gl, ogl = glyphs(A, sigma=(G.DENSE_SIGMA_Y, G.DENSE_SIGMA_Y), max_radius=maxr)
    got, st = gpu_run(A, og, RT["WeightedAverage"], [dict(x=x, y=y, value=v, sigma_x=sx)], glyph=gl, path=2)
    assert_path(st, 2, 3, maxr, covered=False)
    want = O.run(og, RT["WeightedAverage"], x, y, v, glyph=ogl, sigma_x=sx)
    exact = O.run(og, RT["WeightedAverage"], x, y, v, glyph=ogl, wide=True, sigma_x=sx).astype(np.float64)
    assert np.array_equal(np.isnan(want), np.isnan(exact))
    assert_glyph_close(got, want, exact, "split bin", False)
    gotw, _ = gpu_run(A, og, RT["Count"], [dict(x=x, y=y, value=v, sigma_x=sx)], glyph=gl, path=2)
    assert_glyph_close(gotw, O.run(og, RT["Count"], x, y, v, glyph=ogl, sigma_x=sx),
                       O.run(og, RT["Count"], x, y, v, glyph=ogl, wide=True, sigma_x=sx).astype(np.float64), "split bin, weights", False)


# ---- 4. tile side grown at the apron's expense, row bands -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["two_level", "bands"])
def test_tile_side_grown_at_the_aprons_expense(A, few_bins, monkeypatch, mode):
    """160 x 1120 cells with at most 6 bins per pass: 32-cell tiles (5 across) would need 35 row bands, more than the sweep
    takes, so the tile side grows and the apron shrinks below the reach; footprints of up to 65 rows straddle the bands."""
    monkeypatch.setenv("PCR_HIP_DEBUG_TWO_LEVEL", "1" if mode == "two_level" else "0")
    W, H, maxr = 160, 1120, 32.0
    og = O.make_grid((0.0, 0.0, float(W), float(H)))
    rng = np.random.default_rng(41)
    n = 3000
    x, y = rng.uniform(-2.0, W + 2.0, n), rng.uniform(-2.0, H + 2.0, n)
    v = rng.uniform(5.0, 15.0, n).astype(np.float32)
    sx = rng.uniform(4.0, 12.0, n).astype(np.float32)
    gl, ogl = glyphs(A, sigma=(6.0, 6.0), max_radius=maxr)
    got, st = gpu_run(A, og, RT["WeightedAverage"], [dict(x=x, y=y, value=v, sigma_x=sx)], glyph=gl, path=2)
    print("tile", st.lds_tile_w, "apron", st.lds_apron, "bins", st.num_bins)
    assert st.path == 1 and st.lds_tile_w > 32 and st.lds_apron < 32 and st.num_bins > few_bins
    band_rows = st.lds_tile_h * (few_bins // -(-W // st.lds_tile_w))
    rows = np.floor(H - y[(y >= 0) & (y <= H)]).astype(int)
    r = np.array([G.radius_cells(s, maxr) for s in sx[(y >= 0) & (y <= H)]])
    assert r.max() == 32 and np.any((rows // band_rows) != ((rows + r) // band_rows)), "no footprint straddles a band edge"
    want = O.run(og, RT["WeightedAverage"], x, y, v, glyph=ogl, sigma_x=sx)
    exact = O.run(og, RT["WeightedAverage"], x, y, v, glyph=ogl, wide=True, sigma_x=sx).astype(np.float64)
    assert np.array_equal(np.isnan(want), np.isnan(exact))
    assert_glyph_close(got, want, exact, f"grown tile / {mode}", False)


# ---- 5. row-block windows -----------------------------------------------------------------------------------------------------------
class _SplitAt:
    """Stands in for the case's generator where _glyph_shards_add_up draws its split row."""

    def __init__(self, row):
        self.row = row

    def integers(self, lo, hi):
        assert lo <= self.row < hi
        return self.row


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("split", [61, 130], ids=["split-61", "split-through-the-blob"])
def test_row_block_shards_with_a_halo_taller_than_the_apron(A, split, path):
    """Two shards with halo = r + 1 = 49 rows (the LDS apron is 32) add up plane by plane to the unsharded run."""
    W, H, maxr = 200, 260, 48.0
    og = O.make_grid((0.0, 0.0, float(W), float(H)))
    rng = np.random.default_rng(51)
    n = 1200
    x, y = rng.uniform(-2.0, W + 2.0, n), rng.uniform(-2.0, H + 2.0, n)
    x[:n // 2], y[:n // 2] = rng.normal(90.0, 8.0, n // 2), rng.normal(H - 130.0, 6.0, n // 2)     # the blob, around row 130
    v = rng.normal(0.0, 10.0, n).astype(np.float32)
    sx = rng.uniform(10.0, 20.0, n).astype(np.float32)
    assert {G.radius_cells(s, maxr) for s in sx} >= {48} and G.lds_geometry(3, 48)[1] < 48
    blob_rows = np.floor(H - y[:n // 2]).astype(int)
    if split == 130:
        assert (blob_rows < split).sum() > 100 and (blob_rows >= split).sum() > 100
    c = dict(og=og, kind="gauss_chan", rname="WeightedAverage", x=x, y=y, v=v, ch=dict(sigma_x=sx), path=path,
             gl=dict(type=None, sigma_x=9.0, sigma_y=9.0, rotation=0.0, max_radius=maxr), rng=_SplitAt(split))
    _glyph_shards_add_up(A, c)


# ---- 6. non-finite channels at a large radius ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("rname", ["Count", "WeightedAverage", "Sum"])
def test_nonfinite_rotation_and_sigma_channels_at_radius_40(A, rname, path):
    """test_gaussian_nonfinite_rotation_and_sigma_channels at max_radius 40: a NaN / inf rotation paints 81 x 81 NaN weights
    through the float path (the 40-bit fixed-point weight plane cannot hold them), an inf sigma a flat footprint 81 cells wide."""
    og = O.make_grid((0.0, 0.0, 400.0, 300.0), tile=(100, 100))
    rng = np.random.default_rng(77)
    n = 2000
    x, y = rng.uniform(-1.0, 401.0, n), rng.uniform(-1.0, 301.0, n)
    v = rng.uniform(0.5, 2.0, n).astype(np.float32)
    rot = rng.uniform(-3.2, 3.2, n).astype(np.float32)
    inside = np.nonzero((x > 0) & (x < 400) & (y > 0) & (y < 300))[0]
    bad = rng.choice(inside, 11, replace=False)
    rot[bad[:3]] = np.nan
    rot[bad[3]] = np.inf
    rot[bad[4]] = -np.inf
    sig = rng.uniform(8.0, 14.0, n).astype(np.float32)
    sig[bad[5:8]] = np.inf                      # r = min(inf, 40): flat along x
    sig[bad[8:]] = np.nan                       # NaN > 0 is false: default sigma
    gl, ogl = glyphs(A, sigma=(12.0, 9.0), max_radius=40.0)
    ch = dict(rotation=rot, sigma_x=sig)
    assert max(G.radius_cells(s, 40.0) for s in sig[np.isfinite(sig)]) == 40
    got, st = gpu_run(A, og, RT[rname], [dict(x=x, y=y, value=v, **ch)], glyph=gl, path=path)
    if path:
        assert_path(st, path, G.PLANE_MASK[rname], 40.0)
    want = O.run(og, RT[rname], x, y, v, glyph=ogl, **ch)
    exact = O.run(og, RT[rname], x, y, v, glyph=ogl, wide=True, **ch).astype(np.float64)
    assert 5 * 41 * 41 <= np.isnan(want).sum() <= want.size // 2             # the NaN footprints are there, and are not everything
    assert_glyph_close(got, want, exact, f"nonfinite channels r40/{rname}/path {path}", False)
    assert np.isfinite(got[~np.isnan(got)]).all()


# ---- 7. through the Pipeline, Auto path ---------------------------------------------------------------------------------------------
def _pipeline_band(cfg_specs, og, x, y, channels):
    import pcr
    from test_gpu_pipeline_api import cloud_from, config_for
    pipe = pcr.Pipeline.create(config_for(og, cfg_specs, scatter_path=0))
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "hip"
    pipe.ingest(cloud_from(x, y, channels, "device"))
    pipe.finalize()
    return np.array(pipe.result().band_array(0)), pipe.last_scatter()


def test_pipeline_sigma_channel_with_the_default_max_radius():
    import pcr
    og = O.make_grid((0.0, 0.0, 300.0, 220.0), tile=(200, 128))
    rng = np.random.default_rng(71)
    n = 3000
    x, y = rng.uniform(-2.0, 302.0, n), rng.uniform(-2.0, 222.0, n)
    v = rng.uniform(5.0, 15.0, n).astype(np.float32)
    sx = rng.uniform(6.0, 14.0, n).astype(np.float32)
    r = {G.radius_cells(s, 32.0) for s in sx}
    assert max(r) == 32 and min(r) <= 21
    spec = pcr.gaussian_splat_spec("value", sigma_x_channel="sx", default_sigma=5.0)       # max_radius_cells: the default, 32
    assert spec.glyph.max_radius_cells == 32.0
    got, info = _pipeline_band([spec], og, x, y, {"value": v, "sx": sx})
    assert info["path"] == "binned" and info["lds_apron"] == G.lds_geometry(3, 32)[1], info
    ogl = O.make_glyph(GAUSS, sigma_x=5.0, sigma_y=5.0, max_radius=32.0)
    want = O.run(og, O.WEIGHTED_AVERAGE, x, y, v, glyph=ogl, sigma_x=sx)
    exact = O.run(og, O.WEIGHTED_AVERAGE, x, y, v, glyph=ogl, wide=True, sigma_x=sx).astype(np.float64)
    assert_glyph_close(got, want, exact, "pipeline sigma channel r32", False)


def test_pipeline_default_rotation_keeps_a_large_gaussian_off_the_moment_path():
    import pcr
    og = O.make_grid((0.0, 0.0, 300.0, 220.0), tile=(200, 128))
    rng = np.random.default_rng(72)
    n = 3000
    x, y = rng.uniform(-2.0, 302.0, n), rng.uniform(-2.0, 222.0, n)
    v = rng.uniform(5.0, 15.0, n).astype(np.float32)
    spec = pcr.gaussian_splat_spec("value", default_sigma=12.0, default_rotation=0.7, max_radius_cells=48.0)
    got, info = _pipeline_band([spec], og, x, y, {"value": v})
    assert G.radius_cells(12.0, 48.0) == 36
    assert info["path"] == "binned" and info["lds_apron"] == G.lds_geometry(3, 36)[1] < 36, info
    ogl = O.make_glyph(GAUSS, sigma_x=12.0, sigma_y=12.0, rotation=0.7, max_radius=48.0)
    want = O.run(og, O.WEIGHTED_AVERAGE, x, y, v, glyph=ogl)
    exact = O.run(og, O.WEIGHTED_AVERAGE, x, y, v, glyph=ogl, wide=True).astype(np.float64)
    assert_glyph_close(got, want, exact, "pipeline default rotation r36", False)


# ---- 8. the seeded fuzz -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", G.FUZZ_SEEDS)
def test_large_radius_random_case_matches_oracle(A, seed):
    """Comparison and allowances are those of test_gpu_fuzz.test_random_case_matches_oracle; what the 40 seeds cover is
    asserted without a GPU by test_gauss_large_radius_inputs.py."""
    check_case_matches_oracle(A, G.build_case(seed), f"large-radius {seed}")
