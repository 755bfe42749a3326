"""Clouds that sit on the cell edges of a grid, for the tests of the routing (which cell, reference tile, LDS tile, row band
and rank a point belongs to).

The reference floors a TRUE f64 division, floor((wx - min_x) / cell_size_x) (GridConfig::world_to_cell); the device kernels
multiply by 1 / cell_size and divide only when the product lands within a few ulps of an integer (floor_quotient in
csrc/common.hpp).  On a lattice of cell edges -- gridded lidar, coordinates snapped to 0.1 m -- the two formulas floor
differently for hundreds of points; on a uniform random cloud for none.  Every geometry here comes with such a cloud: each
lattice value o + k * cs with its two nextafter neighbours below and above, on either axis and on both at once.

disagreements() is the NumPy restatement of both formulas and cells() of the reference's one; no engine code is used here.
"""
import functools

import numpy as np

import pcr_oracle_py as O

# name -> cell size, origin (min_x, min_y), cells, reference tile, and what differs from a north-up grid with tight bounds
GEOMETRIES = {
    "tenth": dict(cs=0.1, origin=(0.0, 0.0), dims=(1000, 1000), tile=(16, 16)),
    "tenth_one_tile": dict(cs=0.1, origin=(0.0, 0.0), dims=(1000, 1000), tile=(4096, 4096)),
    "seven_tenths": dict(cs=0.7, origin=(0.0, 0.0), dims=(1200, 1200), tile=(10, 10)),
    "third_offset": dict(cs=1.0 / 3.0, origin=(-12.8, 7.3), dims=(900, 640), tile=(50, 50)),
    # a large origin: wx - min_x is a multiple of 2^-34 or so, and the two formulas must not diverge at all
    "utm": dict(cs=1.0 / 3.0, origin=(500000.0, 4649776.22482), dims=(777, 500), tile=(64, 48)),
    "south_up": dict(cs=0.1, origin=(0.0, 0.0), dims=(1000, 256), tile=(64, 64), south_up=True),
    # bounds half a cell beyond the last cell on the max sides: quotients of W and H are reached and must clamp
    "loose_bounds": dict(cs=0.1, origin=(0.0, 0.0), dims=(1000, 1000), tile=(64, 64), loose=0.5),
    # one small tile, for the records of the reference's own glyph code (tests/golden/make_ref_live.py); not in NAMES
    "ref_tile": dict(cs=0.1, origin=(0.0, 0.0), dims=(64, 48), tile=(64, 48), pairs=2000, interior=500),
}
NAMES = [n for n in GEOMETRIES if n != "ref_tile"]
HARD = ["tenth", "seven_tenths"]          # the two the sweep shapes, MostRecent and the row blocks run on

N_PAIRS, N_INTERIOR = 10_000, 2_000


@functools.lru_cache(maxsize=None)
def grid(name):
    """The oracle's grid (pcr_oracle_py.Grid) of a geometry."""
    g = GEOMETRIES[name]
    cs, (ox, oy), (W, H) = g["cs"], g["origin"], g["dims"]
    extra = g.get("loose", 0.0) * cs
    bounds = (ox, oy, ox + W * cs + extra, oy + H * cs + extra)
    return O.make_grid(bounds, cell=(cs, cs if g.get("south_up") else -cs), tile=g["tile"], dims=(W, H))


def _lattice(o, cs, n, lo, hi):
    """o + k * cs for k = 0..n, each with its two nextafter neighbours below and above; those inside [lo, hi]."""
    base = o + np.arange(n + 1, dtype=np.float64) * cs
    d1, u1 = np.nextafter(base, -np.inf), np.nextafter(base, np.inf)
    vals = np.stack([np.nextafter(d1, -np.inf), d1, base, u1, np.nextafter(u1, np.inf)], axis=1).reshape(-1)
    return vals[(vals >= lo) & (vals <= hi)]


def _interior(rng, o, cs, n, count):
    """Coordinates well inside a cell: o + (j + u) * cs, u in [0.25, 0.75]."""
    return o + (rng.integers(0, n, count) + rng.uniform(0.25, 0.75, count)) * cs


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(x, y, value) of a geometry's lattice cloud; the arrays are shared and read-only."""
    og = grid(name)
    g = GEOMETRIES[name]
    cs, (ox, oy), (W, H) = g["cs"], g["origin"], g["dims"]
    n_pairs, n_interior = g.get("pairs", N_PAIRS), g.get("interior", N_INTERIOR)
    rng = np.random.default_rng(list(GEOMETRIES).index(name) + 1)
    lx = _lattice(ox, cs, W, og.min_x, og.max_x)
    ly = _lattice(oy, cs, H, og.min_y, og.max_y)
    pick_x, pick_y = rng.integers(0, len(lx), n_pairs), rng.integers(0, len(ly), n_pairs)
    outside = np.array([np.nextafter(og.min_x, -np.inf), np.nextafter(og.max_x, np.inf)])
    outside_y = np.array([np.nextafter(og.min_y, -np.inf), np.nextafter(og.max_y, np.inf)])
    x = np.concatenate([lx, _interior(rng, ox, cs, W, len(ly)), lx[pick_x], _interior(rng, ox, cs, W, n_interior),
                        outside, _interior(rng, ox, cs, W, 2)])
    y = np.concatenate([_interior(rng, oy, cs, H, len(lx)), ly, ly[pick_y], _interior(rng, oy, cs, H, n_interior),
                        _interior(rng, oy, cs, H, 2), outside_y])
    v = (1 + np.arange(len(x)) % 7).astype(np.float32)     # Sum, Count, Max and Min of these are exact in f32
    for a in (x, y, v):
        a.setflags(write=False)
    return x, y, v


def in_bounds(og, x, y):
    return (x >= og.min_x) & (x <= og.max_x) & (y >= og.min_y) & (y <= og.max_y)


def quotients(og, x, y):
    """Per axis (floor of the true division, floor of the product with the reciprocal), unclamped, as float64."""
    ax, ay = x - og.min_x, y - og.max_y
    div = np.floor(ax / og.cell_size_x), np.floor(ay / og.cell_size_y)
    mul = np.floor(ax * (1.0 / og.cell_size_x)), np.floor(ay * (1.0 / og.cell_size_y))
    return div, mul


def disagreements(og, x, y):
    """(on x, on y): the in-bounds points whose floor(a * (1 / cs)) is not floor(a / cs) on that axis."""
    div, mul = quotients(og, x, y)
    ok = in_bounds(og, x, y)
    return ok & (div[0] != mul[0]), ok & (div[1] != mul[1])


def cells(og, x, y):
    """(col, row, valid) by the reference's formula: inclusive bounds, floor of a true division, clamp."""
    div, _ = quotients(og, x, y)
    col = np.clip(div[0], 0, og.width - 1).astype(np.int64)
    row = np.clip(div[1], 0, og.height - 1).astype(np.int64)
    return col, row, in_bounds(og, x, y)


def on_column_multiple(og, x, y, m):
    """The points that disagree on x across a column that is a multiple of m: one formula says column k * m, the other the
    column before it (m = the reference tile's width, the LDS tile's)."""
    div, mul = quotients(og, x, y)
    return disagreements(og, x, y)[0] & (np.maximum(div[0], mul[0]) % m == 0)


def report(name):
    """One line of counts: what the self-check asserts on, printed by it."""
    og = grid(name)
    x, y, _ = cloud(name)
    dx, dy = disagreements(og, x, y)
    return (f"{name}: {len(x)} points, {int(in_bounds(og, x, y).sum())} in bounds, disagreeing on x {int(dx.sum())} "
            f"({len(np.unique(x[dx]))} values) on y {int(dy.sum())} ({len(np.unique(y[dy]))} values), "
            f"across a column that is a multiple of 10 / 16 / 128: "
            + " / ".join(str(int(on_column_multiple(og, x, y, m).sum())) for m in (10, 16, 128)))
