"""Inputs and restated geometry for the large-radius Gaussian splat tests (test_gpu_gauss_large_radius.py on the GPU,
test_gauss_large_radius_inputs.py for what can be checked without one).  Nothing here touches the device.

The geometry is a restatement, in Python, of what glyph_device.hpp and scatter_binned_glyph.hip do with a point: its
radius, the clip rectangle of the centre cell's reference tile, the clipped window, the form of gauss_splat_wave that
window takes, and the LDS tile / apron glyph_tile picks.  The tests assert from it that the branch they are named for
was taken."""
import functools
import math

import numpy as np

import pcr_oracle_py as O

RADII = (21, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128)
WDT_SET = (1, 42, 63, 64, 65, 127, 128, 129, 191, 192, 193)
HGT_SET = (1, 63, 64, 65, 127, 128, 129, 193)
SUB = (0.3, 0.2)                    # sub-cell position of every isolated centre (sub_cx, sub_cy of gauss_params)
PLANE_MASK = {"Sum": 1, "Count": 2, "Average": 3, "WeightedAverage": 3}
RT = {"Sum": 0, "Average": 3, "WeightedAverage": 4, "Count": 5}


# ---- restated geometry ------------------------------------------------------------------------------------------------
def lds_geometry(mask, need):
    """(tile side S, apron) of glyph_tile for a Gaussian when the grid needs no more than kMaxBands row bands."""
    cell_bytes = (8 if mask & 1 else 0) + (8 if mask & 2 else 0)
    side = int(math.floor(math.sqrt(150 * 1024 // cell_bytes))) & ~1
    S = max(32, min(128, (side - 2 * need) & ~7))
    return S, max(0, min(need, (side - S) // 2))


def item_points(need):
    """Points per work item of binned_glyph for a Gaussian: a bin with more is split among several workgroups."""
    return int(min(65536.0, max(1024.0, 4.0e6 / (2.0 * need + 1.0) ** 2)))


def radius_cells(sx_cells, max_radius):
    """r of gauss_params on a north-up grid: sigma_y / cell_size_y is negative there, so max(sx, sy) is sx."""
    return int(np.ceil(np.minimum(np.float32(3.0) * np.float32(sx_cells), np.float32(max_radius))))


def window(og, col, row, r):
    """(x0, y0, wdt, hgt, cut_by_tile): the (2r+1)^2 window of centre cell (col, row) clipped to its reference tile and
    the grid; cut_by_tile says that a reference-tile edge inside the grid did some of the clipping."""
    cx0 = (col // og.tile_width) * og.tile_width
    cy0 = (row // og.tile_height) * og.tile_height
    cx1, cy1 = min(cx0 + og.tile_width, og.width), min(cy0 + og.tile_height, og.height)
    x0, x1 = max(col - r, cx0), min(col + r + 1, cx1)
    y0, y1 = max(row - r, cy0), min(row + r + 1, cy1)
    cut = ((col - r < cx0 and cx0 > 0) or (col + r + 1 > cx0 + og.tile_width and cx0 + og.tile_width < og.width) or
           (row - r < cy0 and cy0 > 0) or (row + r + 1 > cy0 + og.tile_height and cy0 + og.tile_height < og.height))
    return x0, y0, x1 - x0, y1 - y0, cut


def branch(wdt, hgt, axis_aligned):
    """The form of gauss_splat_wave a window takes."""
    if not axis_aligned or wdt > 192:
        return "generic-div" if wdt * hgt >= (1 << 18) else "generic"
    return "narrow" if wdt <= 64 else "wide"


def centres_to_world(og, cols, rows):
    x = og.min_x + (np.asarray(cols, np.float64) + SUB[0]) * og.cell_size_x
    y = og.max_y - (np.asarray(rows, np.float64) + SUB[1]) * abs(og.cell_size_y)
    return x, y


# ---- parts 1 and 2: isolated footprints ---------------------------------------------------------------------------------
def isolated_cloud(og, pts, ratio=0.8):
    """pts: (col, row, r[, sy/sx[, rotation]]).  sx = r/3 - 0.01 cells, so ceil(3 sx) == r; distinct values."""
    cols, rows = [p[0] for p in pts], [p[1] for p in pts]
    x, y = centres_to_world(og, cols, rows)
    sx = np.array([p[2] / 3.0 - 0.01 for p in pts], np.float32)
    rat = np.array([p[3] if len(p) > 3 else ratio for p in pts], np.float32)
    rot = np.array([p[4] if len(p) > 4 else 0.0 for p in pts], np.float32)
    v = (1.0 + 0.37 * np.arange(len(pts))).astype(np.float32)
    for (c, r_, rr), s in zip([p[:3] for p in pts], sx):
        assert radius_cells(s, 1e9) == rr
        assert O.world_to_cell(og, *[float(a[0]) for a in centres_to_world(og, [c], [r_])])[:2] == (c, r_)
    return dict(x=x, y=y, v=v, sigma_x=sx * np.float32(og.cell_size_x), sigma_y=sx * rat * np.float32(abs(og.cell_size_y)),
                rotation=rot)


def shelf_layout(W, H, radii, gap=2):
    """Unclipped windows side by side, largest first; no two closer than `gap` cells."""
    pts, x, y, shelf = [], 0, 0, 0
    for r in sorted(radii, reverse=True):
        d = 2 * r + 1
        if x + d > W:
            x, y, shelf = 0, y + shelf + gap, 0
        assert x + d <= W and y + d <= H, "shelf layout does not fit"
        pts.append((x + r, y + r, r))
        x, shelf = x + d + gap, max(shelf, d)
    return pts


def centre_for(d, r, t0, t1, from_high):
    """A centre in [t0, t1) whose reach r, clipped to [t0, t1), has extent d -- the first from the named side."""
    for c in (range(t1 - 1, t0 - 1, -1) if from_high else range(t0, t1)):
        if min(c + r + 1, t1) - max(c - r, t0) == d:
            return c
    return None


def tiled_layouts(og, targets, radii=RADII):
    """One point per reference tile (footprints are clipped to the centre's tile, so no two windows touch); every target
    (wdt, hgt) is placed with the first radius, tile and layout that can produce it, the radii tried in rotating order and
    the clipped side alternating.  -> list of layouts, each a list of (col, row, r)."""
    tw, th = og.tile_width, og.tile_height
    tiles = [(tx, ty) for ty in range(-(-og.height // th)) for tx in range(-(-og.width // tw))]
    layouts, used = [], []
    for k, (w, h) in enumerate(targets):
        order = radii[k % len(radii):] + radii[:k % len(radii)]
        spot = None
        for li in range(len(layouts) + 1):
            taken = used[li] if li < len(layouts) else set()
            for tx, ty in tiles:
                if (tx, ty) in taken:
                    continue
                for r in order:
                    c = centre_for(w, r, tx * tw, min(tx * tw + tw, og.width), k % 2 == 1)
                    rw = centre_for(h, r, ty * th, min(ty * th + th, og.height), k % 4 >= 2)
                    if c is not None and rw is not None:
                        spot = (li, tx, ty, c, rw, r)
                        break
                if spot:
                    break
            if spot:
                break
        assert spot, f"no placement for a {w} x {h} window"
        li, tx, ty, c, rw, r = spot
        if li == len(layouts):
            layouts.append([])
            used.append(set())
        layouts[li].append((c, rw, r))
        used[li].add((tx, ty))
    return layouts


GRID_ONE_TILE = dict(bounds=(0.0, 0.0, 1000.0, 800.0), tile=(4096, 4096))
GRID_A = dict(bounds=(0.0, 0.0, 1025.0, 769.0), tile=(256, 256))      # last tile column 1 wide, last tile row 1 tall
GRID_B = dict(bounds=(0.0, 0.0, 833.0, 831.0), tile=(256, 256))       # last tile column 65 wide, last tile row 63 tall
TARGETS_A = [(1, 193), (193, 1), (1, 129), (64, 65), (1, 65), (127, 1), (1, 1), (42, 1), (42, 63), (63, 64), (191, 1),
             (65, 127), (127, 128), (128, 129), (129, 193), (191, 193), (192, 127), (193, 128), (65, 63), (64, 42),
             (129, 128), (193, 193), (63, 42), (128, 65), (192, 192), (65, 129)]
TARGETS_B = [(65, 193), (192, 63), (65, 129), (193, 63), (65, 128), (129, 63), (65, 65), (128, 63), (65, 63), (191, 63),
             (65, 127), (127, 63), (64, 63), (65, 64)]


@functools.lru_cache(maxsize=None)
def part1_cases():
    """-> [(name, grid kwargs, pts)]: the unclipped radii in one reference tile, then the clipped layouts."""
    out = [("unclipped", GRID_ONE_TILE, tuple(shelf_layout(1000, 800, RADII)))]
    for gname, grid, targets in (("A", GRID_A, TARGETS_A), ("B", GRID_B, TARGETS_B)):
        og = O.make_grid(grid["bounds"], tile=grid["tile"])
        for k, pts in enumerate(tiled_layouts(og, targets)):
            out.append((f"clipped{gname}{k}", grid, tuple(pts)))
    return out


GRID_GENERIC = (0.0, 0.0, 640.0, 600.0)
_ROT4 = ((21, 1.0 / 3.0, 0.3), (33, 0.5, -1.1), (64, 0.8, 0.7), (96, 1.0 / 3.0, 2.5))


def _rot_pts(rot=None):
    base = shelf_layout(640, 600, [p[0] for p in _ROT4])
    by_r = {p[0]: p for p in _ROT4}
    return tuple((c, rw, r, by_r[r][1], by_r[r][2] if rot is None else rot) for c, rw, r in base)


# name, reference tile, points, default rotation, rotation channel?, max_radius, branches the windows must take
PART2_CASES = [
    dict(name="rotation_channel", tile=(4096, 4096), pts=_rot_pts(), def_rot=0.0, rot_chan=True, maxr=130.0, want={"generic"}),
    dict(name="default_rotation", tile=(4096, 4096), pts=_rot_pts(0.0), def_rot=0.7, rot_chan=False, maxr=130.0, want={"generic"}),
    dict(name="unrotated_wdt_over_192", tile=(4096, 4096), pts=tuple(shelf_layout(640, 600, (97, 128))), def_rot=0.0,
         rot_chan=False, maxr=130.0, want={"generic"}),
    dict(name="r255_float_row_index", tile=(4096, 4096), pts=((300, 300, 255),), def_rot=0.0, rot_chan=False, maxr=320.0,
         want={"generic"}, dims=(511, 511)),
    dict(name="r256_integer_division", tile=(4096, 4096), pts=((300, 300, 256),), def_rot=0.0, rot_chan=False, maxr=320.0,
         want={"generic-div"}, dims=(513, 513)),
    dict(name="r256_rotated", tile=(4096, 4096), pts=((300, 300, 256, 0.5, 0.7),), def_rot=0.0, rot_chan=True, maxr=320.0,
         want={"generic-div"}, dims=(513, 513)),
    dict(name="clip_600x430_below_2p18", tile=(600, 430), pts=((300, 215, 300),), def_rot=0.0, rot_chan=False, maxr=320.0,
         want={"generic"}, dims=(600, 430)),
    dict(name="clip_600x440_above_2p18", tile=(600, 440), pts=((300, 220, 300),), def_rot=0.0, rot_chan=False, maxr=320.0,
         want={"generic-div"}, dims=(600, 440)),
]


def case_is_rotated(case):
    return case["rot_chan"] or case["def_rot"] != 0.0


def contributed(band):
    """Cells that received a contribution: Sum leaves 0 in an empty cell of a touched tile, the others NaN."""
    return ~np.isnan(band) & (band != 0)


# ---- part 3: dense overlap ------------------------------------------------------------------------------------------------
DENSE_GRID = (300, 220)
# (max_radius, reduction, the LDS apron covers the reach): 16 B/cell windows have side 96, 8 B/cell ones 138
DENSE_CASES = [(32.0, "WeightedAverage", True), (33.0, "WeightedAverage", False),
               (53.0, "Sum", True), (53.0, "Count", True), (54.0, "Sum", False), (54.0, "Count", False),
               (64.0, "Sum", False), (64.0, "Count", False), (64.0, "WeightedAverage", False),
               (96.0, "Sum", False), (96.0, "Count", False), (96.0, "WeightedAverage", False)]
DENSE_SIGMA_Y = 10.0                # cells


def dense_grid(tile, cell=(1.0, -1.0), origin=(0.0, 0.0)):
    W, H = DENSE_GRID
    og = O.make_grid((origin[0], origin[1], origin[0] + W * cell[0], origin[1] + H * abs(cell[1])), cell=cell, tile=tile)
    assert (og.width, og.height) == (W, H)
    return og


@functools.lru_cache(maxsize=None)
def dense_points(seed=31, n=1500):
    """In CELL units (fractional column, fractional row from the top), to be mapped onto a grid by dense_cloud.
    Sum values: mostly in [5, 15], one in ten in [-1.5, -0.5] -- both signs, but where many footprints meet the sum stays
    far from zero, so the bar's floor (1e-3 of the value scale 10) is never asked of a heavily cancelled float32 sum."""
    rng = np.random.default_rng(seed)
    W, H = DENSE_GRID
    fx, fy = rng.uniform(-3.0, W + 3.0, n), rng.uniform(-3.0, H + 3.0, n)        # a few of them outside
    k = n // 2
    fx[:k], fy[:k] = rng.normal(0.55 * W, 9.0, k), rng.normal(0.45 * H, 7.0, k)  # the blob
    sx = rng.uniform(8.0, 22.0, n).astype(np.float32)
    v_pos = rng.uniform(5.0, 15.0, n).astype(np.float32)
    v_sum = v_pos.copy()
    neg = rng.uniform(size=n) < 0.1
    v_sum[neg] = -rng.uniform(0.5, 1.5, int(neg.sum())).astype(np.float32)
    return fx, fy, sx, v_sum, v_pos


def dense_cloud(og, rname):
    fx, fy, sx, v_sum, v_pos = dense_points()
    x = og.min_x + fx * og.cell_size_x
    y = og.max_y - fy * abs(og.cell_size_y)
    return dict(x=x, y=y, value=v_sum if rname == "Sum" else v_pos, sigma_x=sx * np.float32(og.cell_size_x))


# ---- part 8: the seeded fuzz ------------------------------------------------------------------------------------------------
FUZZ_SEEDS = range(40)
FUZZ_CELL_BUDGET = 4.0e7             # window cells per oracle run: ~0.3 s, four runs per case


def build_case(seed):
    """A case of the large-radius space from its seed alone, in the shape of test_gpu_fuzz.build_case."""
    rng = np.random.default_rng(77000 + seed)
    W, H = int(rng.integers(120, 521)), int(rng.integers(100, 421))
    csx = float(rng.choice([0.5, 1.0, 2.5]))
    csy = -float(rng.choice([0.5, 1.0, 2.5])) if seed % 3 == 0 else -csx
    ox, oy = float(rng.choice([0.0, -1234.5, 5e5])), float(rng.choice([0.0, 777.25, 4.1e6]))
    tile = (int(rng.choice([96, 200, 257, 4096])), int(rng.choice([80, 128, 301, 4096])))
    og = O.make_grid((ox, oy, ox + W * csx, oy + H * abs(csy)), cell=(csx, csy), tile=tile)
    assert (og.width, og.height) == (W, H)
    n = int(rng.integers(200, 1501))
    maxr = float(rng.choice([24.0, 32.0, 33.0, 48.0, 64.0, 100.0, 130.0]))
    sxc, syc = float(rng.uniform(7.0, 40.0)), float(rng.uniform(7.0, 40.0))
    rot = float(rng.choice([0.0, 0.0, 0.7, -2.0]))
    ch_sx = rng.uniform(-2.0, 40.0, 1501).astype(np.float32) if rng.uniform() < 0.6 else None
    ch_sy = rng.uniform(3.0, 40.0, 1501).astype(np.float32) if rng.uniform() < 0.3 else None
    ch_rot = rng.uniform(-3.2, 3.2, 1501).astype(np.float32) if rng.uniform() < 0.3 else None
    rname = str(rng.choice(["Sum", "Average", "WeightedAverage", "Count"]))
    path = int(rng.choice([0, 1, 2]))
    # thinned by the generator, not skipped: the oracle's cost is the number of window cells
    reach = min(maxr, 3.0 * (40.0 if ch_sx is not None else sxc))
    n = max(200, min(n, int(FUZZ_CELL_BUDGET / (2.0 * math.ceil(reach) + 1.0) ** 2)))
    mx, my = 3 * csx, 3 * abs(csy)
    x = rng.uniform(og.min_x - mx, og.max_x + mx, n)
    y = rng.uniform(og.min_y - my, og.max_y + my, n)
    if rng.uniform() < 0.5:                                      # clustered half
        k = n // 2
        x[:k] = rng.normal(og.min_x + 0.3 * W * csx, 6 * csx, k)
        y[:k] = rng.normal(og.min_y + 0.6 * H * abs(csy), 6 * abs(csy), k)
    x[:4] = [og.min_x, og.max_x, og.max_x, og.min_x]             # the inclusive corners
    y[:4] = [og.min_y, og.max_y, og.min_y, og.max_y]
    v = rng.normal(0.0, 10.0, n).astype(np.float32)
    ch = {}
    if ch_sx is not None:
        ch["sigma_x"] = ch_sx[:n] * np.float32(csx)               # entries <= 0 take the default
    if ch_sy is not None:
        ch["sigma_y"] = ch_sy[:n] * np.float32(abs(csy))
    if ch_rot is not None:
        ch["rotation"] = ch_rot[:n]
    gl = dict(type=None, sigma_x=sxc * csx, sigma_y=syc * abs(csy), rotation=rot, max_radius=maxr)
    ogl = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=gl["sigma_x"], sigma_y=gl["sigma_y"], rotation=rot, max_radius=maxr)
    return dict(og=og, kind="gauss_chan" if ch else "gauss", rname=rname, x=x, y=y, v=v, ch=ch, gl=gl, ogl=ogl, path=path, rng=rng)


def classify(c):
    """What a fuzz case exercises, from the restated geometry: a set of names."""
    og, gl, ch = c["og"], c["gl"], c["ch"]
    icsx = np.float32(1.0 / og.cell_size_x)
    sxw = np.full(len(c["x"]), gl["sigma_x"], np.float32)
    if "sigma_x" in ch:
        sxw = np.where(ch["sigma_x"] > 0, ch["sigma_x"], sxw).astype(np.float32)
    r = np.ceil(np.minimum(np.float32(3.0) * (sxw * icsx), np.float32(gl["max_radius"]))).astype(int)
    aligned_default = "rotation" not in ch and gl["rotation"] == 0.0
    tags = set()
    for i in range(len(c["x"])):
        col, row, ok = O.world_to_cell(og, float(c["x"][i]), float(c["y"][i]))
        if not ok:
            continue
        _, _, wdt, hgt, cut = window(og, col, row, int(r[i]))
        b = branch(wdt, hgt, aligned_default)
        if b == "wide":
            tags.add("wide form")
        if b in ("wide", "narrow") and hgt > 64:
            tags.add("hgt > 64")
        if not aligned_default and r[i] > 20:
            tags.add("rotated generic")
        if wdt > 192:
            tags.add("wdt > 192")
        if cut:
            tags.add("clipped at a reference-tile edge")
    # the binned path: forced, or Auto on a glyph the moment path cannot take with enough points to be worth the sweep
    binned = c["path"] == 2 or (c["path"] == 0 and (ch or gl["rotation"] != 0.0) and len(c["x"]) * 64 >= og.width * og.height)
    if binned:
        mask = PLANE_MASK[c["rname"]]
        need = math.ceil(gl["max_radius"]) if ("sigma_x" in ch or "sigma_y" in ch) else \
            int(np.ceil(min(np.float32(3.0) * np.float32(gl["sigma_x"]) * icsx, np.float32(gl["max_radius"]))))
        if need > lds_geometry(mask, need)[1]:
            tags.add("spill live with both planes" if mask == 3 else "spill live with one plane")
    return tags


FUZZ_TAGS = ("wide form", "hgt > 64", "rotated generic", "wdt > 192", "spill live with both planes",
             "spill live with one plane", "clipped at a reference-tile edge")
