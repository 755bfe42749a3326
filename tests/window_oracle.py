"""The oracle on one cell window of a large grid: only the points whose footprint can reach the window are run.

    exact, single = window(grid, rtype, x, y, value, (r0, r1, c0, c1), glyph=..., direction=...)

`exact` is the window of `pcr_oracle_py.run(..., wide=True)` (double accumulation: the reference that sums are measured
against), `single` the window of the float32 form (where the NaN masks come from), both (r1 - r0, c1 - c0) float32 and
equal, bit for bit, to the same window of a run over the whole cloud (tests/test_window_oracle.py).

A point reaches the cells within `reach()` of its centre cell -- clipped to the reference tile that holds its routed cell
(Q4) -- so it is selected when its centre cell lies in the window grown by that margin AND its routed tile overlaps the
window.  x, y, value and the glyph channels are numpy arrays or CUDA torch tensors: a cloud that lives on the device is
masked there and only the selected points are copied to the host.  The oracle's grid is the caller's, truncated after the
last reference tile the window touches (the same origin, cell size and tiles: the same arithmetic, a smaller band)."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pcr_oracle_py as O


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def reach(grid, glyph=None, half_length=None):
    """Cells a footprint can extend beyond its centre cell (oracle/pcr_oracle.c, gaussian_one / line_one).
      Point     0
      Gaussian  ceil(min(3 max(sx, sy), max_radius)) with sx, sy the sigmas in cells -- sy is negative on a north-up grid,
                so the reference sizes the footprint by sx there (its std::max)
      Line      round(c + h) for a centre c in [0, 1) and h = min(half length in cells, max_radius) per axis: floor(h + 1/2)
                + 1 cells toward larger indices (the walk's end points are round()ed, the centre cell is floor()ed)
    half_length: the largest per-point half length, when the cloud carries that channel."""
    if glyph is None or glyph.type == O.GLYPH_POINT:
        return 0
    f = np.float32
    inv_x, inv_y = f(1.0 / grid.cell_size_x), f(1.0 / grid.cell_size_y)
    cap = f(glyph.max_radius_cells)
    if glyph.type == O.GLYPH_GAUSSIAN:
        sx, sy = f(glyph.default_sigma_x) * inv_x, f(glyph.default_sigma_y) * inv_y
        r = min(f(3.0) * max(sx, sy), cap)
        return max(0, int(math.ceil(r)))
    if glyph.type == O.GLYPH_LINE:
        hl = f(glyph.default_half_length if half_length is None else half_length)
        h = max(abs(min(hl * inv_x, cap)), abs(min(hl * inv_y, cap)))
        return int(math.floor(float(h) + 0.5)) + 1
    raise ValueError(f"unknown glyph type {glyph.type}")


def _cells(xp, grid, x, y):
    """-> (routed col, routed row, valid, centre col, centre row): pcro_world_to_cell (inclusive bounds, floor of the true
    division, clamped) and the glyph kernels' floor((x - min_x) * (1 / cell size))."""
    valid = (x >= grid.min_x) & (x <= grid.max_x) & (y >= grid.min_y) & (y <= grid.max_y)
    col = xp.clip(xp.floor((x - grid.min_x) / grid.cell_size_x), 0, grid.width - 1)
    row = xp.clip(xp.floor((y - grid.max_y) / grid.cell_size_y), 0, grid.height - 1)
    ccol = xp.floor((x - grid.min_x) * (1.0 / grid.cell_size_x))
    crow = xp.floor((y - grid.max_y) * (1.0 / grid.cell_size_y))
    return col, row, valid, ccol, crow


def select(grid, x, y, win, margin, point=False):
    """Mask (numpy, or a torch tensor on x's device) of the points whose footprint can reach win = (r0, r1, c0, c1) when
    it extends `margin` cells beyond the centre cell.  point: the Point glyph, whose one cell is the routed (clamped) cell."""
    xp = _xp(x)
    r0, r1, c0, c1 = win
    col, row, valid, ccol, crow = _cells(xp, grid, x, y)
    if point:
        ccol, crow = col, row
    tw, th = grid.tile_width, grid.tile_height
    tc0, tr0 = xp.floor(col / tw) * tw, xp.floor(row / th) * th      # the routed tile's first cell (Q4 clips to this tile)
    return (valid & (ccol >= c0 - margin) & (ccol < c1 + margin) & (crow >= r0 - margin) & (crow < r1 + margin)
            & (tc0 < c1) & (tc0 + tw > c0) & (tr0 < r1) & (tr0 + th > r0))


def _touched(grid, x, y, win):
    """Reference tiles overlapping win that hold a valid point of the WHOLE cloud, as {(tile row, tile col)}: an empty cell
    of a touched tile holds 0 in a Sum band, of an untouched one NaN (Q2 / Q3)."""
    xp = _xp(x)
    r0, r1, c0, c1 = win
    col, row, valid, _, _ = _cells(xp, grid, x, y)
    tw, th = grid.tile_width, grid.tile_height
    ta, tb = r0 // th, (r1 - 1) // th
    tl, tr = c0 // tw, (c1 - 1) // tw
    trow, tcol = xp.floor(row / th), xp.floor(col / tw)
    inside = valid & (trow >= ta) & (trow <= tb) & (tcol >= tl) & (tcol <= tr)
    key = (trow[inside] - ta) * (tr - tl + 1) + (tcol[inside] - tl)
    keys = key.unique() if _is_torch(key) else np.unique(key)
    keys = keys.cpu().numpy() if _is_torch(keys) else keys
    return {(ta + int(k) // (tr - tl + 1), tl + int(k) % (tr - tl + 1)) for k in keys}


def _xp(a):
    if _is_torch(a):
        import torch
        return torch
    return np


def _host(a, mask):
    if a is None:
        return None
    a = a[mask]
    return a.cpu().numpy() if _is_torch(a) else np.asarray(a)


def _truncated(grid, win):
    """The caller's grid ending after the last reference tile that win touches: same origin (min_x, max_y), cell size and
    tiles, so every point of those tiles routes, clips and splats as on the whole grid."""
    r1, c1 = win[1], win[3]
    w = min(grid.width, -(-c1 // grid.tile_width) * grid.tile_width)
    h = min(grid.height, -(-r1 // grid.tile_height) * grid.tile_height)
    g = O.Grid(grid.min_x, grid.max_y - h * abs(grid.cell_size_y), grid.min_x + w * abs(grid.cell_size_x), grid.max_y,
               grid.cell_size_x, grid.cell_size_y, w, h, grid.tile_width, grid.tile_height)
    if w == grid.width:
        g.max_x = grid.max_x                                          # not truncated: the caller's own bound, bit for bit
    if h == grid.height:
        g.min_y = grid.min_y
    return g


def window(grid, rtype, x, y, value, win, glyph=None, margin=None, **channels):
    """(exact, single): the window win = (r0, r1, c0, c1) of the oracle, double- and single-accumulated.  margin=None is
    reach(grid, glyph, ...); a smaller one is for showing that the margin is needed."""
    r0, r1, c0, c1 = win
    assert 0 <= r0 < r1 <= grid.height and 0 <= c0 < c1 <= grid.width, win
    assert grid.cell_size_x > 0 > grid.cell_size_y, "north-up grids (cell_size_y < 0) only"
    if margin is None:
        hl = channels.get("half_length")
        hl = None if hl is None or len(hl) == 0 else float(hl.max())
        margin = reach(grid, glyph, hl)
    mask = select(grid, x, y, win, margin, point=glyph is None or glyph.type == O.GLYPH_POINT)
    xs, ys, vs = _host(x, mask), _host(y, mask), _host(value, mask)
    ch = {k: _host(a, mask) for k, a in channels.items()}
    g = _truncated(grid, win)
    with ThreadPoolExecutor(2) as ex:                                 # (ctypes calls release the GIL)
        out = list(ex.map(lambda wide: O.run(g, rtype, xs, ys, vs, glyph=glyph, wide=wide, **ch)[r0:r1, c0:c1],
                          (True, False)))
    if rtype == O.SUM:
        th, tw = grid.tile_height, grid.tile_width
        for tr, tc in _touched(grid, x, y, win):
            rs = slice(max(tr * th, r0) - r0, min((tr + 1) * th, r1) - r0)
            cs = slice(max(tc * tw, c0) - c0, min((tc + 1) * tw, c1) - c0)
            for a in out:
                blk = a[rs, cs]
                blk[np.isnan(blk)] = 0.0
    return out[0], out[1]
