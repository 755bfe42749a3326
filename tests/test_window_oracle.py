"""tests/window_oracle.py against the oracle over the whole cloud: on small grids whose reference tiles are smaller than the
grid (so that the Q4 clip acts), the helper's window equals the same window of a full run bit for bit -- double and single
accumulation, NaN masks included -- at a grid corner, at a grid edge and across reference-tile boundaries; and for every
glyph a point placed exactly `reach` cells from the window shows that a margin one cell smaller loses it."""
import numpy as np
import pytest

import pcr_oracle_py as O
import window_oracle as WO

GLYPHS = {
    # the bench's settings (bench.py make_specs): max_radius 4 sigma capped at 64, 12 for sigma = 4; Line hl + 2
    "point": (None, {}),
    "gauss1": (O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.0, sigma_y=1.0, max_radius=4.0), {}),
    "gauss4": (O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=4.0, sigma_y=4.0, max_radius=12.0), {}),
    "gauss16": (O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=16.0, sigma_y=16.0, max_radius=64.0), {}),
    "line16": (O.make_glyph(O.GLYPH_LINE, half_length=16.0, max_radius=18.0), {"direction": True}),
}
REACH = {"point": 0, "gauss1": 3, "gauss4": 12, "gauss16": 48, "line16": 17}
RTYPES = {"point": (O.SUM, O.COUNT, O.AVERAGE, O.MAX, O.MIN), "line16": (O.WEIGHTED_AVERAGE, O.SUM, O.COUNT)}
# (grid width, height, tile width, height, points): tiles smaller than the grid and not dividing it
SHAPE = {"point": (200, 160, 64, 48, 20_000), "gauss1": (200, 160, 64, 48, 6_000), "gauss4": (200, 160, 64, 48, 3_000),
         "gauss16": (300, 260, 128, 112, 600), "line16": (200, 160, 64, 48, 6_000)}


def _cloud(name, seed, n=None):
    W, H, _, _, npts = SHAPE[name]
    n = npts if n is None else n
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    x[:4], y[:4] = (0.0, W, 0.0, W), (0.0, H, H, 0.0)                  # on the bounds: inclusive, clamped into the last cell
    x[4], y[4] = W + 0.5, H / 2                                       # outside: not valid
    v = rng.uniform(-1, 1, n).astype(np.float32)
    ch = {"direction": rng.uniform(0, np.pi, n).astype(np.float32)} if GLYPHS[name][1].get("direction") else {}
    return x, y, v, ch


def _grid(name):
    W, H, tw, th, _ = SHAPE[name]
    return O.make_grid((0.0, 0.0, float(W), float(H)), tile=(tw, th))


def _windows(name):
    W, H, tw, th, _ = SHAPE[name]
    return {"corner": (0, 24, 0, 30),
            "edge": (H // 2 - 10, H // 2 + 12, W - 26, W),              # the last tile column is a partial tile
            "bottom_right": (H - 20, H, W - 20, W),
            "tile_cross": (th - 9, th + 11, tw - 12, tw + 7),           # four reference tiles meet inside
            "tile_row": (2 * th - 5, 2 * th + 6, 3, W - 3)}


def _full(g, rtype, x, y, v, glyph, ch):
    return [O.run(g, rtype, x, y, v, glyph=glyph, wide=w, **ch) for w in (True, False)]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_reach_is_the_oracles_footprint():
    g = O.make_grid((0.0, 0.0, 64.0, 64.0))
    for name, (glyph, _) in GLYPHS.items():
        assert WO.reach(g, glyph) == REACH[name], name
    # sigma 1.8 / 2 at r <= 7.2 / 8 (bench.py gauss1.8, gauss2): 3 sigma = 5.4 / 6 -> 6
    assert WO.reach(g, O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.8, sigma_y=1.8, max_radius=7.2)) == 6
    assert WO.reach(g, O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=2.0, sigma_y=2.0, max_radius=8.0)) == 6
    # capped by max_radius; on a north-up grid sigma_y does not size the footprint (the reference's std::max(sx, sy))
    assert WO.reach(g, O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=4.0, sigma_y=4.0, max_radius=5.5)) == 6
    assert WO.reach(g, O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.0, sigma_y=9.0, max_radius=64.0)) == 3
    # the Line's cap applies per axis to the signed half extent: on a north-up grid hy = -16 is never above it
    assert WO.reach(g, O.make_glyph(O.GLYPH_LINE, half_length=16.0, max_radius=10.0)) == 17
    assert WO.reach(g, O.make_glyph(O.GLYPH_LINE, half_length=2.5, max_radius=18.0), half_length=7.6) == 9


@pytest.mark.parametrize("name", list(GLYPHS))
def test_window_equals_the_full_run_bit_for_bit(name):
    glyph, _ = GLYPHS[name]
    g = _grid(name)
    x, y, v, ch = _cloud(name, seed=7)
    for rtype in RTYPES.get(name, (O.WEIGHTED_AVERAGE, O.SUM)):
        full = _full(g, rtype, x, y, v, glyph, ch)
        for wname, win in _windows(name).items():
            r0, r1, c0, c1 = win
            got = WO.window(g, rtype, x, y, v, win, glyph=glyph, **ch)
            sel = WO.select(g, x, y, win, WO.reach(g, glyph), point=glyph is None)
            assert 0 < sel.sum() < len(x), (name, wname)
            for form, a, b in zip(("wide", "single"), got, full):
                assert _same(a, b[r0:r1, c0:c1]), f"{name} {O.RTYPE_NAMES[rtype]} {wname} ({form}) differs from the full run"
            assert not np.isnan(got[1]).all(), (name, wname)


@pytest.mark.parametrize("name", list(GLYPHS))
def test_a_margin_one_cell_short_loses_a_point(name):
    """A point whose centre cell lies exactly reach() cells left of the window, with its footprint's nearest reach pointing
    into the window's first column: the window with the margin equals the full run, one cell less does not."""
    glyph, _ = GLYPHS[name]
    g = _grid(name)
    W, H, tw, th, _ = SHAPE[name]
    m = REACH[name]
    x, y, v, ch = _cloud(name, seed=11, n=200)
    c0 = tw + m + 2                                                    # the point and the window share a reference tile
    win = (th + 4, th + 14, c0, c0 + 10)
    px, py = c0 - m + 0.9, H - (th + 8 + 0.5)                          # centre cell (th + 8, c0 - m), sub-cell (0.9, 0.5)
    x, y = np.append(x, px), np.append(y, py)
    v = np.append(v, np.float32(0.75))
    if ch:
        ch = {"direction": np.append(ch["direction"], np.float32(0.0))}   # horizontal: ends at fcx + 16 = c0 - 0.1 -> c0
    rtype = O.SUM if name == "point" else O.WEIGHTED_AVERAGE
    r0, r1, c0_, c1 = win
    full = [b[r0:r1, c0_:c1] for b in _full(g, rtype, x, y, v, glyph, ch)]
    ok = WO.window(g, rtype, x, y, v, win, glyph=glyph, margin=m, **ch)
    short = WO.window(g, rtype, x, y, v, win, glyph=glyph, margin=m - 1, **ch)
    assert all(_same(a, b) for a, b in zip(ok, full))
    assert not any(_same(a, b) for a, b in zip(short, full)), f"{name}: a margin of {m - 1} cells lost nothing"


def test_sum_window_in_a_tile_touched_only_from_outside_it():
    """Q2 / Q3 on a sparse cloud: an empty cell of a reference tile that holds a point is 0 in a Sum band, of an untouched
    tile NaN -- also when the only point of the tile lies outside the window (and so is not selected)."""
    g = O.make_grid((0.0, 0.0, 200.0, 160.0), tile=(64, 48))
    x, y = np.array([5.5, 150.2]), np.array([160.0 - 5.5, 160.0 - 100.5])    # cells (5, 5): tile (0, 0); (100, 150): (2, 2)
    v = np.array([2.0, 3.0], dtype=np.float32)
    win = (10, 60, 10, 80)                                                # tiles (0, 0), (0, 1), (1, 0), (1, 1)
    assert WO.select(g, x, y, win, 0).sum() == 0                          # no point inside: nothing to run
    full = _full(g, O.SUM, x, y, v, None, {})
    got = WO.window(g, O.SUM, x, y, v, win)
    for a, b in zip(got, full):
        assert _same(a, b[10:60, 10:80])
        assert (a[:38, :54] == 0).all()                                   # rows 10..47, cols 10..63: tile (0, 0)
        assert np.isnan(a[38:, :]).all() and np.isnan(a[:, 54:]).all()


def test_device_tensors_select_like_numpy():
    torch = pytest.importorskip("torch")
    g = _grid("gauss4")
    glyph, _ = GLYPHS["gauss4"]
    x, y, v, _ = _cloud("gauss4", seed=3)
    win = _windows("gauss4")["tile_cross"]
    want = WO.window(g, O.WEIGHTED_AVERAGE, x, y, v, win, glyph=glyph)
    got = WO.window(g, O.WEIGHTED_AVERAGE, torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(v), win, glyph=glyph)
    assert all(_same(a, b) for a, b in zip(got, want))
    m = WO.select(g, torch.from_numpy(x), torch.from_numpy(y), win, 12)
    assert np.array_equal(m.numpy(), WO.select(g, x, y, win, 12))
