"""What the large-radius Gaussian tests (test_gpu_gauss_large_radius.py) assume about their own inputs, checked on the
CPU: the layouts reach the window shapes and branches they are meant to, the 1e-6 cut-off is dead where the comparison
is exact, the float32 and the binary64 oracle agree on the mask where a mask allowance is used, and the fuzz generator
covers every branch of the large-radius space at least three times and stays cheap for the oracle."""
import time

import numpy as np
import pytest

import pcr_oracle_py as O
import gauss_large_radius_common as G


def _windows(og, pts):
    return [G.window(og, p[0], p[1], p[2]) for p in pts]


def test_part1_layouts_cover_the_window_shapes():
    cases = G.part1_cases()
    name, grid, pts = cases[0]
    og = O.make_grid(grid["bounds"], tile=grid["tile"])
    assert sorted(p[2] for p in pts) == sorted(G.RADII)
    assert all((w, h) == (2 * p[2] + 1, 2 * p[2] + 1) and not cut for p, (_, _, w, h, cut) in zip(pts, _windows(og, pts)))
    pairs, radii, forms = set(), set(), set()
    for name, grid, pts in cases[1:]:
        og = O.make_grid(grid["bounds"], tile=grid["tile"])
        seen = set()
        for p, (x0, y0, w, h, _) in zip(pts, _windows(og, pts)):
            tile = (p[0] // og.tile_width, p[1] // og.tile_height)
            assert tile not in seen, "two footprints in one reference tile"
            seen.add(tile)
            pairs.add((w, h))
            radii.add(p[2])
            forms.add((G.branch(w, h, True), h > 64))
    assert {w for w, _ in pairs} >= set(G.WDT_SET) and {h for _, h in pairs} >= set(G.HGT_SET)
    assert radii == set(G.RADII)
    assert any(w >= 3 * h and w > 64 for w, h in pairs), "no wide-and-short window"
    assert any(h >= 3 * w and h > 64 for w, h in pairs), "no narrow-and-tall window"
    # every form of gauss_splat_wave with and without a refreshed row table
    assert forms >= {("narrow", False), ("narrow", True), ("wide", False), ("wide", True), ("generic", False), ("generic", True)}
    # the narrow form with one row per step (33 <= wdt <= 64), and two and three column blocks with a ragged last one
    assert any(33 <= w <= 64 for w, _ in pairs)
    assert any(65 <= w <= 128 and w % 64 for w, _ in pairs) and any(129 <= w <= 192 and w % 64 for w, _ in pairs)


@pytest.mark.parametrize("case", G.part1_cases(), ids=lambda c: c[0])
def test_part1_cut_off_is_dead(case):
    name, grid, pts = case
    og = O.make_grid(grid["bounds"], tile=grid["tile"])
    cl = G.isolated_cloud(og, pts)
    ogl = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.0, sigma_y=1.0, max_radius=130.0)
    ch = dict(sigma_x=cl["sigma_x"], sigma_y=cl["sigma_y"])
    w64 = O.run(og, O.COUNT, cl["x"], cl["y"], np.ones(len(pts), np.float32), glyph=ogl, wide=True, **ch)
    w32 = O.run(og, O.COUNT, cl["x"], cl["y"], np.ones(len(pts), np.float32), glyph=ogl, **ch)
    assert np.nanmin(w64) > 2e-6
    assert np.array_equal(G.contributed(w64), G.contributed(w32))
    assert int(G.contributed(w64).sum()) == sum(w * h for _, _, w, h, _ in _windows(og, pts))


@pytest.mark.parametrize("case", G.PART2_CASES, ids=lambda c: c["name"])
def test_part2_windows_take_the_generic_loop(case):
    og = O.make_grid(G.GRID_GENERIC, tile=case["tile"])
    assert (og.width, og.height) == (640, 600)
    wins = _windows(og, case["pts"])
    assert {G.branch(w, h, not G.case_is_rotated(case)) for _, _, w, h, _ in wins} == case["want"]
    if "dims" in case:
        assert [(w, h) for _, _, w, h, _ in wins] == [case["dims"]]
    for a in range(len(wins)):                                       # isolated: no two windows touch
        for b in range(a):
            xa, ya, wa, ha, _ = wins[a]
            xb, yb, wb, hb, _ = wins[b]
            assert xa >= xb + wb or xb >= xa + wa or ya >= yb + hb or yb >= ya + ha
    cl = G.isolated_cloud(og, case["pts"])
    ogl = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.0, sigma_y=1.0, rotation=case["def_rot"], max_radius=case["maxr"])
    ch = dict(sigma_x=cl["sigma_x"], sigma_y=cl["sigma_y"])
    if case["rot_chan"]:
        ch["rotation"] = cl["rotation"]
    ones = np.ones(len(case["pts"]), np.float32)
    w64 = O.run(og, O.COUNT, cl["x"], cl["y"], ones, glyph=ogl, wide=True, **ch)
    w32 = O.run(og, O.COUNT, cl["x"], cl["y"], ones, glyph=ogl, **ch)
    assert np.array_equal(np.isnan(w64), np.isnan(w32)), "the two oracles disagree on the mask"
    if not G.case_is_rotated(case):
        assert np.nanmin(w64) > 2e-6
        assert int(G.contributed(w64).sum()) == sum(w * h for _, _, w, h, _ in wins)


def test_lds_geometry_at_its_edges():
    # both planes: 16 B/cell, side 96; one plane: 8 B/cell, side 138
    assert G.lds_geometry(3, 32) == (32, 32) and G.lds_geometry(3, 33) == (32, 32)
    assert G.lds_geometry(1, 53) == (32, 53) and G.lds_geometry(2, 54) == (32, 53)
    assert G.lds_geometry(3, 64)[1] == 32 and G.lds_geometry(1, 96)[1] == 53


@pytest.mark.parametrize("tile", [(4096, 4096), (200, 128)])
def test_dense_case_oracles_agree_on_the_mask(tile):
    og = G.dense_grid(tile)
    for maxr, rname, _ in G.DENSE_CASES:
        if rname == "Sum":
            continue                                                 # (no NaN inside a touched tile)
        cl = G.dense_cloud(og, rname)
        ogl = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=G.DENSE_SIGMA_Y, sigma_y=G.DENSE_SIGMA_Y, max_radius=maxr)
        a = O.run(og, G.RT[rname], cl["x"], cl["y"], cl["value"], glyph=ogl, sigma_x=cl["sigma_x"])
        b = O.run(og, G.RT[rname], cl["x"], cl["y"], cl["value"], glyph=ogl, wide=True, sigma_x=cl["sigma_x"])
        assert np.array_equal(np.isnan(a), np.isnan(b))
        m = ~np.isnan(b)
        assert np.max(np.abs(a[m].astype(np.float64) - b[m]) / np.maximum(1e-3, np.abs(b[m]))) < 1e-5


def test_fuzz_generator_covers_the_large_radius_space():
    count = {t: 0 for t in G.FUZZ_TAGS}
    paths, rnames = set(), set()
    for seed in G.FUZZ_SEEDS:
        c = G.build_case(seed)
        c2 = G.build_case(seed)
        assert np.array_equal(c["x"], c2["x"]) and c["path"] == c2["path"], "a case must follow from its seed alone"
        assert 200 <= len(c["x"]) <= 1500 and 120 <= c["og"].width <= 520 and 100 <= c["og"].height <= 420
        for t in G.classify(c):
            count[t] += 1
        paths.add(c["path"])
        rnames.add(c["rname"])
    assert all(v >= 3 for v in count.values()), count
    assert paths == {0, 1, 2} and rnames == {"Sum", "Average", "WeightedAverage", "Count"}


def test_fuzz_cases_are_cheap_for_the_oracle():
    """The costliest seed by window cells: one float32 and one binary64 oracle run well inside the two seconds a case may
    spend on its four runs."""
    def cost(c):
        n, r = len(c["x"]), min(c["gl"]["max_radius"], 3.0 * (40.0 if "sigma_x" in c["ch"] else c["gl"]["sigma_x"] / c["og"].cell_size_x))
        return n * (2 * r + 1) ** 2
    c = max((G.build_case(s) for s in G.FUZZ_SEEDS), key=cost)
    assert cost(c) <= 1.05 * max(G.FUZZ_CELL_BUDGET, 200 * 261.0 ** 2)
    t0 = time.perf_counter()
    for wide in (False, True):
        O.run(c["og"], G.RT[c["rname"]], c["x"], c["y"], c["v"], glyph=c["ogl"], wide=wide, **c["ch"])
    assert time.perf_counter() - t0 < 2.0                            # (0.2 s where this was written)
