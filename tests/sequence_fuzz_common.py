"""Operation-sequence fuzz of one pipeline against an exact model (tests/test_sequence_fuzz_host.py on the host engine,
tests/test_gpu_sequence_fuzz.py on the HIP engine).

build(seed) draws a grid, a set of Point reductions, a finalize plan and a SEQUENCE of operations on one pipeline: ingests of
every kind, finalizes between them, plane and touched-flag pointers handed out (and written through), flag unions, checkpoints
that a new pipeline with another plan or flavour resumes from (or that a later load_state lays over whatever the state is
then).  check_sequence() runs the sequence and compares, after every
finalize, every band the pipeline hands out with the Model below, bit for bit and NaN payloads included.  No tolerance is
needed because of how the values are chosen: channel `a` holds multiples of 1/8, channel `b` small integers, and the generator
itself checks that no cell's sum of magnitudes reaches 2^24 units over all clouds of the case -- every partial sum is exact in
binary32 in any order, Average is one binary32 division of two exact numbers, Max / Min / MostRecent select.

The generator uses NumPy only (a seed means the same case on every machine).  The model uses no engine code except the host
twins of the finishing steps, which the CPU suite holds to their own NumPy models: pcr.ground_filter, pcr.fill_nodata,
overviews_common.pyramid; and the `.pcrt` writer for the reference checkpoint.

Every finalize plan also draws PipelineConfig::terrain (0 to 6 entries on any band that leaves, _draw_terrain): the model
appends those bands by terrain_common.terrain, the NumPy restatement of the contract -- not pcr.terrain, so that the host-engine
run holds the host loop's plumbing to something that shares no code with it.  Since every source band is exact here, the
terrain bands of an Average source are held to the model on both engines too.

Line cases: a seed from LINE_SEED_BASE on appends Line-glyph reductions (Sum, Count, Average, WeightedAverage; plane masks 1, 2
and 3; one glyph or two that differ in one parameter) and maybe a Point WeightedAverage to what the seed draws, gives every
cloud a `dir` and an `hl` channel, and may replace clouds by a hot Line tile or by late-large values for a packed item
(_line_pass, last and from generators of its own: a seed below LINE_SEED_BASE stays the case it is).  A Line visit has weight
1, so with these values a group's sum plane is an exact sum and its weight plane an integer: the model adds the oracle's
footprint (oracle/pcr_oracle.c through pcr_oracle_py, the one thing here that is not NumPy) in binary64 and needs no
tolerance.  _line_pass checks the exactness condition for the Line sums with the oracle's binary64 mode on |v| and thins a
cloud that would break it.  Gaussian groups are not drawn: their weights are expf values and their sums depend on the order
of addition.

Accumulator cases: a seed from ACC_SEED_BASE on is what the Point-only generator draws for it, in core, plus (_acc_pass and
_acc_tables, last and from generators of their own) a float32 channel `z` of arbitrary values on every cloud, surface channels,
a filter of its own on reductions and accumulator entries, histograms, extremes and cell-stats entries, tree bands, zonal
tables, and the ops read_acc, tables and set_zones.  `z` and the surface channels feed selections (Max, Min, MostRecent) and
accumulators only, whose states are integers and whose bands are defined bit by bit: the model is the *_common model of each
feature on the same routing, the host twin for the tree bands, zonal_common's Python ints for the tables -- no tolerance.
save_state and load_state are refused while an accumulator list is non-empty: the ops stay, must raise, and move nothing.

Polygon cases: a seed from POLY_SEED_BASE on is what the accumulator generator draws for seed - POLY_SEED_BASE + ACC_SEED_BASE
plus (_poly_pass, last and from generators of its own) 1 to 3 polygon channels with one or two polygon sets each, a use of
every channel -- in PipelineConfig::filter, in the filters of reductions and accumulator entries, as the value of a Max, Min or
filtered Count, as a histogram's channel, as a label -- 1 to 3 point zonal entries, a `lab` channel, points outside the grid and
inside a polygon in every cloud, and the ops set_polygons, point_tables, set_zones_poly, polygonize and reburn.  The model of a
polygon channel is points_in_polygons_common.model with the set that is current at the ingest; of a point zonal table
point_zonal_common.table_masked on the concatenated points of every ingest that counted (the contract: the bits depend on the
multiset of points only); of a burnt label grid rasterize_common.model; of an outline polygonize_common.model.  The reburn chain
needs no model: a zonal entry whose zones were burnt from polygonize(tree_id) answers the by-band entry's table, bit for bit."""
import filecmp
import os

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
TYPES = ("Sum", "Count", "Average", "Max", "Min", "MostRecent")
MAX_FINALIZE_OUTPUTS = 8                   # PCR_HIP_MAX_FINALIZE_OUTPUTS: a larger group flushes in the middle
EXACT_UNITS = 1 << 23                      # the clouds stay below this per cell and channel (units: 1/8 for `a`, 1 for `b`)
PATCH_UNITS = 64                           # a plane patch adds at most this many units to a cell: k/8 on an `a` plane, an integer on a `b` or Count plane
SPLIT_RECORDS = 1 << 17                    # kPointItemRecords: the scan splits a bin that holds more records
HOT_W, HOT_H = 128, 56                     # every Point LDS tile is 128 columns wide and at least 56 rows tall (20 B per cell), from cell (0, 0)
FILL_TYPES = ("Average", "WeightedAverage", "Max", "Min", "MostRecent")     # fill_nodata.h: fills_nodata
OPS8 = ("Equal", "NotEqual", "Less", "LessEqual", "Greater", "GreaterEqual", "InSet", "NotInSet")
# planes a reduction needs / its checkpoint holds, as slots (0 sum, 1 count, 2 max, 3 min; MostRecent: 0 value, 1 timestamp)
PLANES_OF = {"Sum": (0,), "Count": (1,), "Max": (2,), "Min": (3,), "Average": (0, 1), "WeightedAverage": (0, 1), "MostRecent": (0, 1)}
# Line cases: a seed from LINE_SEED_BASE on appends Line-glyph reductions (and maybe a Point WeightedAverage) to what the seed
# draws anyway, from generators of their own (_line_pass); a seed below it stays the case it is
LINE_SEED_BASE = 2000
LINE_TYPES = ("Sum", "Count", "Average", "WeightedAverage")    # pipeline_common.h: glyph_reduction_ok
LINE_MAX_RADIUS = (2.0, 16.0, 32.0)
LINE_CORNER = 32                           # no Line LDS tile is smaller than 32 x 32 cells (glyph_tile): a corner of one tile whatever the glyph
LINE_ITEM_RECORDS = 65535                  # binned_glyph's item_points: k_tile_line_rec counts a cell's visits in 16 bits
LINE_LONG_CELLS = 40000.0                  # a half_length beyond the int16 offsets of the end-point records: the listed path (k_line_list)
# k_tile_line_rec's LDS layout (csrc/scatter_binned_glyph.hip): count plane from byte 16, sum plane from byte 65 528, the list of
# left-out segments between them; at most 12 288 cells; packed words (both planes kept) accept 8 exponents
LINE_COUNT_BASE, LINE_SUM_BASE, LINE_MAX_CELLS, LINE_PACKED_WINDOW = 16, 65528, 12288, 7
# PipelineConfig::terrain: the products by terrain_product_name in TerrainProduct's order, and parameters that create accepts
TERRAIN_PRODUCTS = ("slope", "slope_percent", "aspect", "hillshade", "tri", "tpi", "roughness")
TERRAIN_Z = (1.0, 1.0, 2.0, 0.37)
TERRAIN_LIGHTS = ((315.0, 45.0), (90.0, 30.0), (10.0, 80.0), (200.0, 60.0))

# Seeds of the suite.  (a failing seed of a soak joins the list with a one-line comment)
# 0..31, and the further seeds that the situations and the marks of tests/test_sequence_fuzz_host.py needed more of; 75 is a
# second seed on which import_window without its bands_stale() fails
FIRST_SEEDS = list(range(32)) + [47, 48, 49, 51, 54, 64, 75, 76]     # (tests/golden/sequence_fuzz_cases.json pins what they mean)
# ... and the seeds that the terrain situations needed more of (TERRAIN_SITUATIONS below)
DEFAULT_SEEDS = FIRST_SEEDS + [
    34,     # terrain of hag (none of the seeds before draws it), of the filled dtm and of a Min band, fill 3, in core
    80,    # terrain bands in a GeoTIFF with a write_cog level; a terrain source in a group of 10 outputs, after a plane write
    100,    # slope of the filled dtm (fill 8); two tri bands of one Count band under two names
    123,    # out of core: terrain of hag with fill 3, finalized five times between merges
    181,    # a slope_percent, aspect, hillshade (light 200 / 60) launch on a Sum band in a group of 10 outputs, Device result
    255,    # 520 x 512 out of core: terrain bands in the write_cog level, hillshade second of its launch
    265,    # write_cog level; the resuming pipeline's plan drops the five terrain bands
    280,    # out of core: terrain of dtm with fill, a launch with its hillshade last, finalized again after load_state
    538,    # the loading pipeline's plan turns hag and fill on: terrain of hag, Device result, another terrain list
    640,    # terrain of a band that the first ingest stored, the finalize right behind it; hillshade not first of its launch
    1076,   # terrain of a stored band, finalize right behind the first ingest, then again after a plane write
    1088,   # terrain of a stored band and of the filled dtm, finalize right behind the first ingest
]


def seeds_from_env(name="PCR_SEQ_FUZZ_SEEDS"):
    env = os.environ.get(name)
    if env and ":" in env:
        a, b = env.split(":")
        return list(range(int(a), int(b)))
    if env:
        return [int(v) for v in env.split(",")]
    return list(DEFAULT_SEEDS) + list(LINE_SEEDS) + list(ACC_SEEDS) + list(POLY_SEEDS)


# ---- the generator (NumPy only; a line case: and the oracle) ------------------------------------------------------------------------------------------------
def cells_of(g, x, y):
    """Flat cell of every point by the oracle's world_to_cell (inclusive bounds, floor of the TRUE binary64 division, clamp),
    -1 outside the bounds.  The same IEEE operations as oracle/pcr_oracle.c, vectorised; the host test checks it against
    pcr_oracle_py.world_to_cell point by point on a sample."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ok = (x >= g["min_x"]) & (x <= g["max_x"]) & (y >= g["min_y"]) & (y <= g["max_y"])
    col = np.clip(np.floor((x - g["min_x"]) / g["cs"]), 0, g["W"] - 1).astype(np.int64)
    row = np.clip(np.floor((y - g["max_y"]) / -g["cs"]), 0, g["H"] - 1).astype(np.int64)
    return np.where(ok, row * g["W"] + col, -1)


def groups_of(specs):
    """Accumulation groups as every engine forms them (pipeline_common.h: same_group): same value channel through the same
    glyph -- every parameter of it, same_glyph -- (MostRecent: and timestamp channel, a group of its own) under the same
    ReductionSpec::filter (an accumulator case: the same predicates in the same order)."""
    groups = []
    for i, s in enumerate(specs):
        gl = s.get("glyph")
        key = (s["ch"], s["type"] == "MostRecent", None if gl is None else tuple(sorted(gl.items())), filter_key(s.get("filt")))
        for gr in groups:
            if gr["key"] == key:
                break
        else:
            gr = dict(key=key, ch=s["ch"], select=key[1], glyph=gl, slots=set(), outs=[], filt=s.get("filt"))
            groups.append(gr)
        gr["slots"].update(PLANES_OF[s["type"]])
        gr["outs"].append(i)
        s["group"] = groups.index(gr)
    return groups


def _draw_plan(rng, specs, ooc, big):
    types = [s["type"] for s in specs]
    ground = None
    if "Min" in types:
        kind = str(rng.choice(["off", "dtm", "hag"], p=[0.4, 0.3, 0.3]))
        if kind == "hag" and "Max" not in types:
            kind = "dtm"
        if kind != "off":
            ground = dict(source=types.index("Min"), top=types.index("Max") if kind == "hag" else None, maxr=int(rng.choice([4, 8])))
    out = bool(rng.uniform() < (0.8 if big else 0.3))
    return dict(fill=int(rng.choice([0, 0, 1, 3, 8])), ground=ground,
                loc="Host" if ooc else str(rng.choice(["Host", "Device"])), out=out, cog=out and bool(rng.uniform() < (0.9 if big else 0.5)))


def terrain_band_name(t):
    return t["name"] or f"{t['source']}_{t['product']}"


def _draw_terrain(rng, specs, plan, more=()):
    """PipelineConfig::terrain of a plan: 0 to 6 entries (none in four plans of ten), each a product of any band that leaves
    under the plan.  Half of the entries copy source, z_factor and compute_edges from the entry before, so that launches of
    several products form -- also ones whose Hillshade entry is not the first and has a light of its own.  Every entry draws
    all its numbers, used or not: what one entry draws does not move the next.  `more`: an accumulator case's percentile,
    extremes and Mean bands."""
    sources = [band_name(i, s) for i, s in enumerate(specs)] + list(more)
    if plan["ground"]:
        sources += ["dtm"] + (["hag"] if ground_names(specs, plan)[1] is not None else [])
    n = 0 if rng.uniform() < 0.4 else int(rng.integers(1, 7))
    out, taken = [], set(sources)
    for k in range(n):
        share = bool(rng.uniform() < 0.5) and k > 0
        source, product = sources[int(rng.integers(0, len(sources)))], TERRAIN_PRODUCTS[int(rng.integers(0, 7))]
        z, edges = TERRAIN_Z[int(rng.integers(0, 4))], bool(rng.uniform() < 0.5)
        azimuth, altitude = TERRAIN_LIGHTS[int(rng.integers(0, 4))]
        explicit = bool(rng.uniform() < 1 / 3)
        if share:
            source, z, edges = out[-1]["source"], out[-1]["z_factor"], out[-1]["edges"]
        t = dict(source=source, product=product, name="", z_factor=z, edges=edges, azimuth=azimuth, altitude=altitude)
        if explicit or terrain_band_name(t) in taken:                # (the same source and product under another light or z_factor)
            t["name"] = f"t{k}"
        taken.add(terrain_band_name(t))
        out.append(t)
    return out


def terrain_launches(terrain):
    """plan_terrain's launches: entries that share source, z_factor and compute_edges and name different products, each entry
    into the first launch that takes it.  -> lists of indices"""
    launches = []
    for i, t in enumerate(terrain):
        for l in launches:
            f = terrain[l[0]]
            if (f["source"], f["z_factor"], f["edges"]) == (t["source"], t["z_factor"], t["edges"]) and \
                    all(terrain[m]["product"] != t["product"] for m in l):
                l.append(i)
                break
        else:
            launches.append([i])
    return launches


def _draw_flavour(rng):
    ooc = bool(rng.uniform() < 0.25)
    return dict(ooc=ooc, bands=int(rng.choice([2, 3])), host_budget=int(rng.choice([1, 1 << 30])))


def _draw_cloud(rng, g, shape, filt=None):
    W, H, cs = g["W"], g["H"], g["cs"]
    n = int(rng.integers(1, 60001))
    if shape == "all":                                           # one cell beyond the bounds, and onto them
        x, y = rng.uniform(g["min_x"] - cs, g["max_x"] + cs, n), rng.uniform(g["min_y"] - cs, g["max_y"] + cs, n)
        k = n // 12
        x[:k] = rng.choice([g["min_x"], g["max_x"]], k)
        y[k:2 * k] = rng.choice([g["min_y"], g["max_y"]], k)
    elif shape == "strip":                                       # a few rows
        y0 = rng.uniform(g["min_y"], g["max_y"])
        x, y = rng.uniform(g["min_x"], g["max_x"], n), rng.uniform(y0, min(g["max_y"], y0 + 6 * cs), n)
    elif shape == "cluster":                                     # on a reference-tile corner
        cx = g["min_x"] + min(g["tw"], W) * cs * int(rng.integers(0, max(1, W // g["tw"]) + 1))
        cy = g["max_y"] - min(g["th"], H) * cs * int(rng.integers(0, max(1, H // g["th"]) + 1))
        x, y = rng.normal(cx, 6 * cs, n), rng.normal(cy, 6 * cs, n)
    elif shape == "outside":
        x, y = rng.uniform(g["max_x"] + cs, g["max_x"] + 50 * cs, n), rng.uniform(g["min_y"], g["max_y"], n)
    elif shape == "hot":                                         # > 2^17 points inside the first 128 x 56 cells: one LDS tile of any group
        n = SPLIT_RECORDS + int(rng.integers(2000, 9000))
        x = rng.uniform(g["min_x"], g["min_x"] + min(W, HOT_W) * cs, n)
        y = rng.uniform(g["max_y"] - min(H, HOT_H) * cs, g["max_y"], n)
    else:                                                        # "empty"
        n = 0
        x = y = np.zeros(0)
    t = rng.integers(0, 6, n).astype(np.float32)                 # many ties
    if n:
        idx = rng.integers(0, n, n // 20 + 1)
        t[idx] = np.array([np.nan, -FLT_MAX], np.float32)[rng.integers(0, 2, len(idx))]
    cls = rng.integers(0, 4, n).astype(np.float32)
    if shape == "hot":                                           # the records must reach the bin: classes the filter keeps
        kept = np.arange(4, dtype=np.float32)[keep_mask(filt, np.arange(4, dtype=np.float32))]
        cls = kept[rng.integers(0, len(kept), n)]
    return dict(shape=shape, x=x, y=y, a=(rng.integers(-512, 513, n) / 8.0).astype(np.float32),
                b=rng.integers(0, 4096, n).astype(np.float32), t=t, cls=cls)


def hot_records(case, c):
    """Records of a cloud that reach the first LDS tile of every group (columns < 128, rows < 56) past the filter and the bounds."""
    g = case["grid"]
    cell = cells_of(g, c["x"], c["y"])
    ok = keep_mask(case["filt"], c["cls"]) & (cell >= 0)
    return int((ok & (cell // g["W"] < HOT_H) & (cell % g["W"] < HOT_W)).sum())


CLOUD_KEYS = ("x", "y", "a", "b", "t", "cls")
LINE_CLOUD_KEYS = ("dir", "hl")            # only the clouds of a line case have them


ACC_CLOUD_KEYS = ("z",)                    # ... and only the clouds of an accumulator case this one


POLY_CLOUD_KEYS = ("lab",)                 # ... and the clouds of a polygon case with a point zonal entry by `lab` this one


def cloud_keys(c):
    return CLOUD_KEYS + (LINE_CLOUD_KEYS if "dir" in c else ()) + (ACC_CLOUD_KEYS if "z" in c else ()) + (POLY_CLOUD_KEYS if "lab" in c else ())


def _thin(c, keep):
    for k in cloud_keys(c):
        c[k] = c[k][keep]


def point_units(g, clouds):
    """Per channel (`a` in units of 1/8, `b` in units of 1) and cell, the sum of |v| over the points of the clouds whose centre
    cell it is: what a Point group's sum plane can reach at most.  -> (2, W * H)"""
    units = np.zeros((2, g["W"] * g["H"]))
    for c in clouds:
        cell = cells_of(g, c["x"], c["y"])
        m = cell >= 0
        units[0] += np.bincount(cell[m], np.abs(c["a"][m].astype(np.float64)) * 8.0, g["W"] * g["H"])
        units[1] += np.bincount(cell[m], c["b"][m].astype(np.float64), g["W"] * g["H"])
    return units


# ---- line cases --------------------------------------------------------------------------------------------------------------
def oracle_grid(g):
    import pcr_oracle_py as O
    og = O.make_grid((g["min_x"], g["min_y"], g["max_x"], g["max_y"]), cell=(g["cs"], -g["cs"]), tile=(g["tw"], g["th"]))
    assert (og.width, og.height) == (g["W"], g["H"])
    return og


def oracle_line(og, gl, rtype, c, ch_values, sel, wide=False):
    """One oracle band of the points `sel` of a cloud through the Line glyph `gl`: the footprint of the model."""
    import pcr_oracle_py as O
    kw = dict(direction=c["dir"][sel])
    if gl["hl_ch"]:
        kw["half_length"] = c["hl"][sel]
    ogl = O.make_glyph(O.GLYPH_LINE, half_length=gl["hl"], max_radius=gl["maxr"])
    return O.run(og, rtype, c["x"][sel], c["y"][sel], ch_values[sel], glyph=ogl, wide=wide, **kw)


def line_tile(g, gl, mask):
    """glyph_tile and binned_glyph of csrc/scatter_binned_glyph.hip for a Line glyph on a grid that one sweep bins: the side S of
    the LDS tiles (they start at cell (0, 0) of an in-core pipeline), the apron, whether the walk-state records and
    k_tile_line_rec are used, and how many left-out segments that kernel's list holds."""
    f32 = np.float32
    cell_bytes = (8 if mask & 1 else 0) + (4 if mask & 2 else 0)
    side = int(np.floor(np.sqrt(150 * 1024 // max(cell_bytes, 4)))) & ~1
    cap = min(max(gl["maxr"], 0.0), 4096.0)
    if gl["hl_ch"]:
        need = int(np.ceil(cap)) + 1
    else:
        hx, hy = f32(gl["hl"]) * f32(1.0 / g["cs"]), f32(gl["hl"]) * f32(-1.0 / g["cs"])
        ax, ay = (cap if h > gl["maxr"] else min(abs(float(h)), 4096.0) for h in (hx, hy))
        need = int(np.ceil(max(ax, ay))) + 1
    S = min(128, (side - 2 * need) & ~7)
    if not gl["hl_ch"] and 110 - 2 * need >= 32:
        S = min(S, (110 - 2 * need) & ~7)
    S = max(S, 32)
    apron = max(0, min(need, (side - S) // 2))
    lw = S + 2 * apron
    rec = apron >= need and not gl["hl_ch"] and lw <= 127 and lw * lw <= LINE_MAX_CELLS
    return dict(S=S, apron=apron, need=need, state_records=rec, list_cap=(LINE_SUM_BASE - LINE_COUNT_BASE) // 4 - lw * lw)


def line_tile_records(case, c, gr):
    """Mask of the records of a cloud that reach the FIRST LDS tile of Line group `gr` of an in-core pipeline: past the filter,
    centre cell inside the bounds and inside [0, S) x [0, S)."""
    g = case["grid"]
    S = line_tile(g, gr["glyph"], sum(1 << p for p in gr["slots"]))["S"]
    cell = cells_of(g, c["x"], c["y"])
    return keep_mask(case["filt"], c["cls"]) & (cell >= 0) & (cell // g["W"] < S) & (cell % g["W"] < S)


def line_list_load(case, c, gr):
    """For a packed k_tile_line_rec item made of the records of line_tile_records: how many of them lie outside the window of
    8 exponents, whichever record's exponent the first 1024 make the window's top (the bins are filled by atomics: no order
    is promised).  -> (fewest, most, list_cap, records), or None where the group is not packed or takes another kernel."""
    t = line_tile(case["grid"], gr["glyph"], sum(1 << p for p in gr["slots"]))
    if gr["slots"] != {0, 1} or not t["state_records"]:
        return None
    m = line_tile_records(case, c, gr)
    v = np.abs(c[gr["ch"]][m])
    e = np.frexp(v[v > 0])[1]
    if len(e) == 0:
        return None
    outs = [int(((e < top - LINE_PACKED_WINDOW) | (e > top)).sum()) for top in np.unique(e)]
    return min(outs), max(outs), t["list_cap"], int(m.sum())


def _draw_line_specs(rl):
    """The reductions a line case appends behind the Point ones: maybe a Point WeightedAverage, then 1 to 4 Line reductions in
    one or two groups whose plane masks are drawn (1: Sum; 2: Count; 3: both planes), through one Line glyph or through two
    that differ in exactly one parameter."""
    out = []
    if rl.uniform() < 0.4:
        out.append(dict(type="WeightedAverage", ch=str(rl.choice(["a", "b"]))))
    gl = dict(hl_ch="hl" if rl.uniform() < 0.4 else "", hl_cells=float(np.round(rl.uniform(0.5, 6.0), 3)),
              maxr=float(rl.choice(LINE_MAX_RADIUS)))
    glyphs = [gl]
    two_groups = bool(rl.uniform() < 0.6)
    if two_groups and rl.uniform() < 0.6:
        which = str(rl.choice(["hl_ch", "hl_cells", "maxr"]))
        other = dict(gl)
        if which == "hl_ch":
            other["hl_ch"] = "" if gl["hl_ch"] else "hl"
        elif which == "hl_cells":
            other["hl_cells"] = float(np.round(gl["hl_cells"] + rl.uniform(0.6, 2.0), 3))
        else:
            other["maxr"] = float(rl.choice([r for r in LINE_MAX_RADIUS if r != gl["maxr"]]))
        glyphs.append(other)
    ch0 = str(rl.choice(["a", "b"]))
    chans = [ch0]
    if two_groups and len(glyphs) == 1:                          # one glyph: the second group is the other channel's
        chans.append("b" if ch0 == "a" else "a")
    elif two_groups and rl.uniform() < 0.7:                      # two glyphs: mostly on ONE channel, so that only same_glyph keeps them apart
        chans.append(ch0)
    elif two_groups:
        chans.append(str(rl.choice(["a", "b"])))
    forms = {1: [["Sum"]], 2: [["Count"]],
             3: [["Average"], ["WeightedAverage"], ["Sum", "Count"], ["WeightedAverage", "Sum"], ["Average", "Count"]]}
    lines = []
    for k, ch in enumerate(chans):
        mask = int(rl.choice([1, 2, 3], p=[0.3, 0.2, 0.5]))
        form = forms[mask][int(rl.integers(0, len(forms[mask])))]
        lines += [dict(type=t, ch=ch, glyph=k if len(glyphs) == 2 else 0) for t in form]
    return out, [lines[i] for i in rl.permutation(len(lines))], glyphs


def _draw_line_channels(rl, g, c):
    """`dir` and `hl` of a cloud (float32, finite): directions in [-7, 7], a share beyond +-64 rad (where line_params_fast
    declines), a share of exact multiples of pi / 4; half lengths of 0 to 8 cells with zeros and negative entries (hy is
    negative on these north-up grids and never capped: quirk Q7), and in some clouds up to 8 entries of 40 000 cells."""
    n, cs = len(c["x"]), g["cs"]
    d = rl.uniform(-7.0, 7.0, n)
    far = rl.uniform(size=n) < 0.1
    d[far] = rl.uniform(64.0, 80.0, int(far.sum())) * rl.choice([-1.0, 1.0], int(far.sum()))
    d[far] = np.where(np.abs(d[far]) <= 64.0, 80.0, d[far])                     # (64, 80]
    diag = rl.uniform(size=n) < 0.1
    d[diag] = rl.integers(-8, 9, int(diag.sum())) * (np.pi / 4)
    hl = rl.uniform(0.0, 8.0, n) * cs
    kind = rl.uniform(size=n)
    hl[kind < 0.1] = 0.0
    hl[kind > 0.9] *= -1.0
    k = int(rl.integers(1, 9)) if rl.uniform() < 0.35 else 0
    if n and k:
        hl[rl.integers(0, n, k)] = LINE_LONG_CELLS * cs
    c["dir"], c["hl"] = d.astype(np.float32), hl.astype(np.float32)


def _draw_line_cloud(rl, g, kind, filt):
    """The clouds only a line case has, all inside the first 32 x 32 cells (one LDS tile of any Line group, in core):
    "hot_line": more than 65 535 records, so the tile is more than one item, small values so that thinning never halves it;
    "late_overflow": ~3000 points with |a| <= 1/4, then as many of |a| = 1/8 and of |a| >= 32 as no list of left-out segments
    holds -- a packed window of 8 exponents leaves one of the two kinds out wherever its top lies, and in the cloud's own
    order the large ones arrive after the window is fixed;  "late_used": the ~3000, then a handful of larger values (half of
    them one exponent above the small ones' window), so that the list is used and never full."""
    cs = g["cs"]
    small = lambda k: rl.integers(-2, 3, k) / 8.0
    sign = lambda k: rl.choice([-1.0, 1.0], k)
    if kind == "hot_line":
        n = LINE_ITEM_RECORDS + int(rl.integers(2000, 9000))
        a = rl.integers(-16, 17, n) / 8.0
    elif kind == "late_overflow":
        cap = (LINE_SUM_BASE - LINE_COUNT_BASE) // 4             # (no list is longer)
        k = cap + cap // 3
        late = np.concatenate([sign(k) / 8.0, sign(k) * rl.integers(256, 513, k) / 8.0])
        a = np.concatenate([small(3000), late[rl.permutation(2 * k)]])
    else:
        k = int(rl.integers(8, 41))
        late = np.concatenate([sign(k) * rl.integers(4, 8, k) / 8.0, sign(k) * rl.integers(256, 513, k) / 8.0])
        a = np.concatenate([small(3000), late[rl.permutation(2 * k)]])
    n = len(a)
    x = rl.uniform(g["min_x"], g["min_x"] + LINE_CORNER * cs, n)
    y = rl.uniform(g["max_y"] - LINE_CORNER * cs, g["max_y"], n)
    if kind == "late_used" and g["W"] >= 48:
        # the handful lies beside the corner, in columns 32 to 87 of the same tile (a tile of k_tile_line_rec is at least 88
        # wide) where nothing else of the cloud falls: in a packed word a value that was wrongly taken into the window is put
        # right by any two other visits of its cell (each adds 2^31 + q > 2^30), so only a cell that it has to itself shows it
        x[3000:] = rl.uniform(g["min_x"] + LINE_CORNER * cs, g["min_x"] + min(g["W"], 88) * cs, n - 3000)
    kept = np.arange(4, dtype=np.float32)[keep_mask(filt, np.arange(4, dtype=np.float32))]
    return dict(shape=kind, x=x, y=y, a=a.astype(np.float32), b=rl.integers(0, 64, n).astype(np.float32),
                t=rl.integers(0, 6, n).astype(np.float32), cls=kept[rl.integers(0, len(kept), n)])


def _line_pass(seed, g, specs, ops, clouds, filt):
    """What makes a seed >= LINE_SEED_BASE a line case, drawn last and from generators of its own (94000, seed, k): k = 0 the
    appended reductions, the plane writes turned onto them and which clouds are replaced by a Line cloud; k = 1 + i the
    replacement and the `dir` / `hl` channels of cloud i.  Then the exactness condition for the Line groups: per group and
    cell, the oracle's binary64 sum of |v| over the footprints of every cloud, plus the patches, stays below 2^24 units --
    a cloud that would break it is thinned."""
    import pcr_oracle_py as O
    rl = np.random.default_rng((94000, seed, 0))
    W, H = g["W"], g["H"]
    point_wa, lines, glyphs = _draw_line_specs(rl)
    for gl in glyphs:                                            # as the ReductionSpec holds it: world units, binary32
        gl["hl"] = float(np.float32(gl.pop("hl_cells") * g["cs"]))
    specs += point_wa + [dict(type=s["type"], ch=s["ch"], glyph=dict(glyphs[s["glyph"]])) for s in lines]
    groups = groups_of(specs)
    # plane writes: most of them go to a plane of an appended reduction (a Line group's sum or weight plane, a WeightedAverage's)
    targets = [i for i, s in enumerate(specs) if "glyph" in s or s["type"] == "WeightedAverage"]
    for k, o in enumerate(ops):
        turn = rl.uniform() < (0.7 if o["op"] == "planes_write" else 0.35 if o["op"] == "planes_read" else 0.0)
        r, h, w = int(rl.choice(targets)), int(rl.integers(1, 21)), int(rl.integers(1, 21))
        r0, c0, u = int(rl.integers(0, H - min(h, H) + 1)), int(rl.integers(0, W - min(w, W) + 1)), int(rl.integers(-PATCH_UNITS, PATCH_UNITS + 1))
        slot = int(rl.choice(PLANES_OF[specs[r]["type"]]))
        if turn:
            value = float(1 + abs(u) % 3) if slot == 1 else float(u) if specs[r]["ch"] == "b" else u / 8.0
            ops[k] = dict(op="planes_write", group=specs[r]["group"], slot=slot, rect=(r0, c0, min(h, H), min(w, W)), value=value)
    # clouds: some are replaced by a Line cloud (never the hot spot of the opening, which the marks are about), all get dir and hl
    for kind in ("hot_line", "late_overflow", "late_used"):
        i = int(rl.integers(0, len(clouds)))
        if rl.uniform() < 0.22 and clouds[i]["shape"] != "hot":
            clouds[i] = dict(shape=kind)
    og = oracle_grid(g)
    line_groups = [gr for gr in groups if gr["glyph"] is not None]
    units = [np.zeros(W * H) for _ in line_groups]
    points = np.zeros((2, W * H))                                # the Point sums too: a replaced cloud is new to them
    for i, c in enumerate(clouds):
        rc = np.random.default_rng((94000, seed, 1 + i))
        if len(c) == 1:
            c = clouds[i] = _draw_line_cloud(rc, g, c["shape"], filt)
        _draw_line_channels(rc, g, c)
        while len(c["x"]):
            inside = cells_of(g, c["x"], c["y"]) >= 0
            mag = {"a": np.abs(c["a"]) * np.float32(8.0), "b": c["b"]}
            new = [u + np.nan_to_num(oracle_line(og, gr["glyph"], O.SUM, c, mag[gr["ch"]], inside, wide=True)).reshape(-1).astype(np.float64)
                   for u, gr in zip(units, line_groups)] if inside.any() else units
            if max(u.max() for u in new) < EXACT_UNITS and (points + point_units(g, [c])).max() < EXACT_UNITS:
                units = new
                break
            _thin(c, np.arange(len(c["x"])) % 2 == 0)
        points += point_units(g, [c])
    patched = PATCH_UNITS * sum(o["op"] == "planes_write" for o in ops)
    assert max(u.max() for u in units) + patched < 1 << 24
    return groups


# ---- accumulator cases ---------------------------------------------------------------------------------------------------------
# A seed from ACC_SEED_BASE on is an accumulator case (never a line case): what the Point-only generator draws for the seed, in
# core, plus -- last and from generators of their own, (95000, seed, k) -- a float32 channel `z` on every cloud, surface channels,
# per-reduction filters, histograms, extremes and cell-stats entries, tree bands and zonal tables, and the ops that read them.
ACC_SEED_BASE = 10000
ACC_ITEM_RECORDS = 1 << 16                 # kHistItemRecords, kExtItemRecords, kStatItemRecords: the scan splits a bin that holds more
ACC_HOT_W, ACC_HOT_H = 128, 8              # every accumulator LDS tile is 128 columns wide and at least 8 rows tall, from cell (0, 0)
HIST_BINS = (1, 8, 37, 256)
ACC_MAX_COUNTERS = 6_000_000               # bins x cells of one cube: 256 bins up to ~150 x 150 cells, 37 up to ~400 x 400
HIST_RANGES = ((-4.0, 28.0), (5.0, 12.0), (-1000.0, 1000.0), (40.0, 50.0))     # inside, narrower than, around and beyond the canopy's values
HIST_QS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
EXT_K = (2, 4, 8)
EXT_GAPS = (0.0, 0.5, 1.0, float("inf"))
STAT_STEPS = ((0.0, 0.01), (-2.0, 2.0 ** -6), (1500.0, 0.001))
STAT_SUFFIX = ("mean", "var", "std")       # CellStat's order
ZONAL_MAX_BINS = 37                        # the Python-int fold walks every bin of every labelled cell
# TreeSpec parameters tests/test_trees.py holds the host twin to the brute-force model with
TREE_KW = (dict(), dict(max_radius_cells=1), dict(max_radius_cells=32, window_base=20.0, window_slope=1.5),
           dict(window_base=0.0, window_slope=0.0), dict(min_height=5.0, min_crown_height=1.0, crown_ratio=0.8, max_crown_radius=3.0),
           dict(crown_ratio=0.0, max_crown_radius=float("inf"), min_crown_height=-5.0),
           dict(min_height=0.5, min_crown_height=0.25, window_base=5.0), dict(min_height=-100.0))
SURFACE_THRESHOLDS = (-120.0, -95.0, 0.0, 2.5, 100.0)


def filter_key(f):
    """What makes two filters equal to same_predicate: the fields a predicate's op uses (the set of InSet / NotInSet, else the value)."""
    return None if not f else tuple((p["ch"], p["op"], tuple(p["set"]) if p["op"] in ("InSet", "NotInSet") else p["value"]) for p in f)


def pred_mask(ch, p):
    """One predicate on float32 values, as NumPy compares them: a NaN fails all but NotEqual and NotInSet."""
    v = np.asarray(ch, np.float32)
    with np.errstate(all="ignore"):
        if p["op"] in ("InSet", "NotInSet"):
            inside = np.isin(v, np.array(p["set"], np.float32))
            return inside if p["op"] == "InSet" else ~inside
        t = np.float32(p["value"])
        return {"Equal": v == t, "NotEqual": v != t, "Less": v < t, "LessEqual": v <= t, "Greater": v > t, "GreaterEqual": v >= t}[p["op"]]


def conj_mask(chans, f, n):
    """AND of a filter's predicates over the channels of a cloud (its surface channels included)."""
    keep = np.ones(n, bool)
    for p in f or ():
        keep &= pred_mask(chans[p["ch"]], p)
    return keep


def surface_of(sc):
    import sample_grid_common as SG
    return SG.make_surface(sc["w"], sc["h"], sc["seed"], csx=sc["csx"], csy=sc["csy"], min_x=sc["min_x"], max_y=sc["max_y"])


def surface_channels(acc, c):
    """The cloud's channels and the surface channels of the case, by sample_grid_common.model."""
    import sample_grid_common as SG
    out = dict(c)
    for sc in acc["surfaces"]:
        out[sc["name"]] = SG.model(surface_of(sc), c["x"], c["y"], c["z"] if sc["value"] else None, sc["mode"]) if len(c["x"]) else np.zeros(0, np.float32)
    return out


def ground_names(specs, plan):
    """(source band, top band or None) of a plan's ground filter: by index into the reductions, or -- an accumulator case --
    by name."""
    gr = plan["ground"]
    if "source_name" in gr:
        return gr["source_name"], gr["top_name"]
    return band_name(gr["source"], specs[gr["source"]]), None if gr["top"] is None else band_name(gr["top"], specs[gr["top"]])


def acc_bands(acc):
    """The accumulator bands in the order they leave, behind the reductions': [(name, kind, entry, index within it)]."""
    out = []
    for i, h in enumerate(acc["hist"]):
        out += [(f"h{i}_p{j}", "percentile", i, j) for j in range(len(h["qs"]))]
    out += [(f"x{i}_{'high' if e['side'] else 'low'}", "extremes", i, 0) for i, e in enumerate(acc["ext"])]
    for i, s in enumerate(acc["stats"]):
        out += [(f"c{i}_{STAT_SUFFIX[p]}", STAT_SUFFIX[p], i, j) for j, p in enumerate(s["products"])]
    return out


def acc_filled(kind):
    """fill_nodata_radius: percentile bands fill like Max, extremes like Min or Max, Mean like Average; Variance and StdDev never."""
    return kind in ("percentile", "extremes", "mean")


def acc_terrain_sources(acc):
    return [name for name, kind, _, _ in acc_bands(acc) if acc_filled(kind)]


def z_field(g, seed):
    """The canopy of a case: Gaussian bumps of height 3..30 and sigma 1.5..5 cells (trees_common.canopy's kind), in cell units."""
    r = np.random.default_rng((95000, seed, 999))
    n = int(min(120, max(3, g["W"] * g["H"] // 400)))
    return r.uniform(0, g["H"], n), r.uniform(0, g["W"], n), r.uniform(3.0, 30.0, n), r.uniform(1.5, 5.0, n)


def _draw_z(rc, g, c, field, shift, specials=1.0):
    """Channel `z` of a cloud: the canopy at the point plus noise (+ shift), float32; then a share of NaN, +-Inf, -0.0,
    denormals, and values far beyond every histogram's [lo, hi) and every cell-stats entry's +-2^21 steps.  No +0.0: the
    engines' Max and Min of -0.0 and +0.0 need not agree on the sign, and with one zero there is nothing to agree on."""
    n = len(c["x"])
    r0, c0, amp, sig = field
    u, v = (c["x"] - g["min_x"]) / g["cs"], (g["max_y"] - c["y"]) / g["cs"]
    z = np.zeros(n)
    for k in range(len(r0)):
        near = (np.abs(v - r0[k]) < 4 * sig[k]) & (np.abs(u - c0[k]) < 4 * sig[k])
        z[near] = np.maximum(z[near], amp[k] * np.exp(-((v[near] - r0[k]) ** 2 + (u[near] - c0[k]) ** 2) / (2.0 * sig[k] ** 2)))
    z = (z + rc.normal(0.0, 0.3, n) + shift).astype(np.float32)
    kind = rc.uniform(size=n) * specials
    z[kind < 0.03] = np.nan
    z[(kind >= 0.03) & (kind < 0.035)] = np.inf
    z[(kind >= 0.035) & (kind < 0.04)] = -np.inf
    z[(kind >= 0.04) & (kind < 0.06)] = np.float32(-0.0)
    den = (kind >= 0.06) & (kind < 0.07)
    z[den] = rc.integers(1, 1 << 23, int(den.sum())).astype(np.uint32).view(np.float32) * rc.choice([-1.0, 1.0], int(den.sum())).astype(np.float32)
    far = (kind >= 0.07) & (kind < 0.08)
    z[far] = (rc.choice([-1.0, 1.0], int(far.sum())) * 10.0 ** rc.uniform(5, 9, int(far.sum()))).astype(np.float32)
    z[z == 0] = np.float32(-0.0)
    c["z"] = z


def kept_classes(filt, *filters):
    """The classes 0..3 that the pipeline filter and the `cls` predicates of every given filter keep."""
    cls = np.arange(4, dtype=np.float32)
    keep = keep_mask(filt, cls)
    for f in filters:
        for p in f or ():
            if p["ch"] == "cls":
                keep &= pred_mask(cls, p)
    return cls[keep]


def acc_entries(acc):
    return [e for kind in ("hist", "ext", "stats") for e in acc[kind]]


def _acc_pass(seed, g, specs, ops, clouds, filt, plan):
    """What makes a seed >= ACC_SEED_BASE an accumulator case, from generators of its own (95000, seed, k): k = 0 the lists
    and the plan, k = 1 + i channel `z` (and maybe the replacement) of cloud i.  -> (groups, acc)"""
    ra = np.random.default_rng((95000, seed, 0))
    W, H, cs = g["W"], g["H"], g["cs"]
    # plane writes name a group: they follow their reduction when the filters regroup the specs
    for o in ops:
        if o["op"] == "planes_write":
            o["spec"] = next(i for i, s in enumerate(specs) if s["group"] == o["group"] and o["slot"] in PLANES_OF[s["type"]]
                             and s["type"] in ("Sum", "Count", "Average"))
        elif o["op"] == "checkpoint":                            # refused: no new pipeline, plan or flavour
            o["plan"] = o["flavour"] = None
    surfaces = []
    if ra.uniform() < 0.4:
        kinds = [("hag", "z"), ("smp", "")]
        two = bool(ra.uniform() < 0.4)
        first = int(ra.uniform() < 0.3)
        for name, value in ([kinds[first], kinds[1 - first]] if two else [kinds[first]]):
            sw, sh = int(ra.integers(8, 41)), int(ra.integers(8, 41))
            surfaces.append(dict(name=name, value=value, mode=int(ra.integers(0, 2)), w=sw, h=sh, seed=int(ra.integers(0, 1 << 30)),
                                 csx=float(W * cs * ra.uniform(0.6, 1.1) / sw), csy=float(-H * cs * ra.uniform(0.6, 1.1) / sh),
                                 min_x=float(g["min_x"] + W * cs * ra.uniform(-0.1, 0.2)), max_y=float(g["max_y"] - H * cs * ra.uniform(-0.1, 0.2))))
    snames = [sc["name"] for sc in surfaces]
    # the filters of the case: a pool of up to 5 conjunctions of 1 to 3 predicates (create's limits: 8 distinct filters, 16
    # predicates per conjunction with the pipeline filter's, 32 in all), so that equal filters -- one class -- occur
    pool = []
    for _ in range(int(ra.integers(1, 6))):
        f = []
        for _ in range(int(ra.integers(1, 4))):
            if snames and ra.uniform() < 0.25:
                f.append(dict(ch=str(ra.choice(snames)), op=str(ra.choice(OPS8)), value=float(ra.choice(SURFACE_THRESHOLDS)),
                              set=[float(v) for v in ra.choice(SURFACE_THRESHOLDS, 2, replace=False)]))
            else:
                f.append(dict(ch="cls", op=str(ra.choice(OPS8)), value=float(ra.integers(0, 4)),
                              set=[float(v) for v in ra.choice(4, int(ra.integers(1, 4)), replace=False)]))
        if filter_key(f) not in [filter_key(q) for q in pool]:
            pool.append(f)
    pick = lambda p: pool[int(ra.integers(0, len(pool)))] if ra.uniform() < p else []
    chan = lambda: str(ra.choice(snames)) if snames and ra.uniform() < 0.35 else "z"
    hist, ext, stats = [], [], []
    counts = [int(ra.integers(0, 4)) for _ in range(3)]
    if sum(counts) == 0:
        counts[int(ra.integers(0, 3))] = 1
    for _ in range(counts[0]):
        lo, hi = HIST_RANGES[int(ra.integers(0, len(HIST_RANGES)))]
        qs = [HIST_QS[i] for i in ra.permutation(len(HIST_QS))[:int(ra.integers(0, 5))]]
        bins = int(ra.choice(HIST_BINS))
        while bins * W * H > ACC_MAX_COUNTERS:                   # (the cube and the model's walk of it stay small: fewer bins on a large grid)
            bins = HIST_BINS[HIST_BINS.index(bins) - 1]
        hist.append(dict(ch=chan(), lo=lo, hi=hi, bins=bins, qs=qs, filt=pick(0.6)))
    for _ in range(counts[1]):
        ext.append(dict(ch=chan(), side=int(ra.integers(0, 2)), k=int(ra.choice(EXT_K)), gap=float(ra.choice(EXT_GAPS)), filt=pick(0.6)))
    for _ in range(counts[2]):
        origin, res = STAT_STEPS[int(ra.integers(0, 3))]
        products = [int(p) for p in ra.permutation(3)[:int(ra.integers(1, 4))]]
        stats.append(dict(ch=chan(), origin=origin, res=res, products=products, ddof=int(ra.integers(0, 2)), filt=pick(0.6)))
    shift = 1500.0 if any(s["origin"] == 1500.0 for s in stats) else 0.0
    for h in hist:
        if h["ch"] == "z":
            h["lo"], h["hi"] = h["lo"] + shift, h["hi"] + shift
    # reductions on `z` and on surface channels: selections only (Max, Min, MostRecent); then every reduction's filter
    for _ in range(int(ra.integers(0, 4))):
        ch = chan()
        specs.append(dict(type=str(ra.choice(["Max", "Min"] if ch != "z" else ["Max", "Min", "MostRecent"])), ch=ch))
    if snames and "hag" in snames and ra.uniform() < 0.5:
        specs.append(dict(type="Max", ch="hag"))                # the canopy height model trees are made for
    for s in specs:
        s["filt"] = pick(0.5)
    groups = groups_of(specs)
    for o in ops:
        if o["op"] == "planes_write":
            o["group"] = specs[o.pop("spec")]["group"]
    acc = dict(surfaces=surfaces, hist=hist, ext=ext, stats=stats, shift=shift)
    distinct = {filter_key(e["filt"]) for e in acc_entries(acc) + specs if e["filt"]}
    assert len(distinct) <= 8 and sum(len(k) for k in distinct) + (1 if filt else 0) <= 32

    # the plan: ground and top may name accumulator bands too
    bands = acc_bands(acc)
    low = [band_name(i, s) for i, s in enumerate(specs) if s["type"] == "Min"] + \
          [n for n, kind, i, _ in bands if kind == "mean" or kind == "percentile" or (kind == "extremes" and not ext[i]["side"])]
    high = [band_name(i, s) for i, s in enumerate(specs) if s["type"] == "Max"] + \
           [n for n, kind, i, _ in bands if kind == "mean" or kind == "percentile" or (kind == "extremes" and ext[i]["side"])]
    if low and ra.uniform() < 0.6:
        hag = bool(high) and bool(ra.uniform() < 0.5)
        plan["ground"] = dict(source_name=str(ra.choice(low)), top_name=str(ra.choice(high)) if hag else None, maxr=int(ra.choice([4, 8])))

    # clouds: maybe a hot accumulator tile, a cloud an entry's filter empties, one the pipeline filter empties; `z` on all
    field = z_field(g, seed)
    filtered = [e for e in acc_entries(acc) if e["filt"]]
    swap = {}
    free = [i for i, c in enumerate(clouds) if c["shape"] != "hot"]
    for kind, p in (("hot_acc", 0.35), ("entry_filtered", 0.35), ("pipeline_filtered", 0.2)):
        if free and ra.uniform() < p:
            swap[free.pop(int(ra.integers(0, len(free))))] = kind
    total = 0
    units = np.zeros((2, W * H))
    for i, c in enumerate(clouds):
        rc = np.random.default_rng((95000, seed, 1 + i))
        kind = swap.get(i)
        target = filtered[int(rc.integers(0, len(filtered)))]["filt"] if filtered else []
        if kind == "hot_acc":                                   # more accepted records in the first 128 x 8 cells than one work item takes
            every = acc_entries(acc)
            keep = kept_classes(filt, every[int(rc.integers(0, len(every)))]["filt"])
            keep = keep if len(keep) else kept_classes(filt)
            n = ACC_ITEM_RECORDS + int(rc.integers(2000, 9000))
            c = clouds[i] = dict(shape=kind, x=rc.uniform(g["min_x"], g["min_x"] + min(W, ACC_HOT_W) * cs, n),
                                 y=rc.uniform(g["max_y"] - min(H, ACC_HOT_H) * cs, g["max_y"], n), cls=keep[rc.integers(0, len(keep), n)])
        elif kind in ("entry_filtered", "pipeline_filtered"):
            cls4 = np.arange(4, dtype=np.float32)
            if kind == "entry_filtered":                        # classes the pipeline filter keeps and the entry's filter drops
                keep = np.setdiff1d(kept_classes(filt), kept_classes(filt, target))
            else:
                keep = cls4[~keep_mask(filt, cls4)]
            if len(keep):
                n = int(np.exp(rc.uniform(0.0, np.log(20000.0))))    # (many small ones: the direct path of an Auto pipeline)
                c = clouds[i] = dict(shape=kind, x=rc.uniform(g["min_x"], g["max_x"], n), y=rc.uniform(g["min_y"], g["max_y"], n),
                                     cls=keep[rc.integers(0, len(keep), n)])
        if "a" not in c:
            n = len(c["x"])
            c.update(a=(rc.integers(-64, 65, n) / 8.0).astype(np.float32), b=rc.integers(0, 64, n).astype(np.float32),
                     t=rc.integers(0, 6, n).astype(np.float32))
        _draw_z(rc, g, c, field, shift, specials=4.0 if c["shape"] == "hot_acc" else 1.0)
        while (units + point_units(g, [c])).max() >= EXACT_UNITS:
            _thin(c, np.arange(len(c["x"])) % 2 == 0)
        units += point_units(g, [c])
        total += len(c["x"])
    # every counter stays below its wrap point (2^32) and S2 exact (below 2^22 accepted points a cell): the whole case is smaller
    assert total < 1 << 22
    return groups, acc


def external_labels(g, lab):
    """An external label grid: zonal_common.plot_labels (plots numbered row-major, a NaN column, the invalid labels in row 0)
    with everything outside a window made no zone -- NaN, 0, a negative, 2.5 in turn."""
    import zonal_common as Z
    out = Z.plot_labels(g["W"], g["H"], lab["plot"])
    r0, c0, h, w = lab["window"]
    inside = np.zeros(out.shape, bool)
    inside[r0:r0 + h, c0:c0 + w] = True
    none = np.array([np.nan, 0.0, -3.0, 2.5], np.float32)[(np.arange(out.size) % 4).reshape(out.shape)]
    return np.where(inside, out, none).astype(np.float32)


def _acc_tables(seed, case):
    """Tree bands and zonal tables of the plan, and the ops that read the accumulators and the tables, from a generator of
    their own (95000, seed, 500): read_acc, tables and set_zones are INSERTED into the sequence ahead of its last finalize."""
    rt = np.random.default_rng((95000, seed, 500))
    g, specs, acc, plan, ops = case["grid"], case["specs"], case["acc"], case["plan"], case["ops"]
    W, H = g["W"], g["H"]
    bands = acc_bands(acc)
    sources = [band_name(i, s) for i, s in enumerate(specs)] + [n for n, _, _, _ in bands]
    if plan["ground"]:
        sources += ["dtm"] + (["hag"] if ground_names(specs, plan)[1] is not None else [])
    canopy = [band_name(i, s) for i, s in enumerate(specs) if s["type"] == "Max" and s["ch"] in ("z", "hag")]
    trees = []
    for k in range(int(rt.choice([0, 1, 2], p=[0.3, 0.45, 0.25]))):
        src = str(rt.choice(canopy)) if canopy and rt.uniform() < 0.5 else sources[int(rt.integers(0, len(sources)))]
        trees.append(dict(source=src, kw=int(rt.integers(0, len(TREE_KW)))))
    plan["trees"] = trees
    zonal, labels = [], []
    folds = [i for i, h in enumerate(acc["hist"]) if h["bins"] <= ZONAL_MAX_BINS]
    if acc["stats"] or folds:
        for k in range(int(rt.choice([0, 1, 2], p=[0.3, 0.4, 0.3]))):
            by_tree = bool(trees) and W * H <= 40000 and bool(rt.uniform() < 0.6)
            if by_tree:
                zones, external = f"t{int(rt.integers(0, len(trees)))}_id", False
            else:
                zones, external = f"plots{len(labels)}", True
                h, w = int(rt.integers(8, min(H, 96) + 1)), int(rt.integers(8, min(W, 96) + 1))
                sets = [dict(plot=int(rt.choice([8, 16, 32])), window=(int(rt.integers(0, H - h + 1)), int(rt.integers(0, W - w + 1)), h, w))
                        for _ in range(1 + int(rt.uniform() < 0.4))]          # (a second set replaces the first)
                labels.append(sets)
            st = [int(rt.integers(0, len(acc["stats"])))] if acc["stats"] and rt.uniform() < 0.8 else []
            hs = [int(rt.choice(folds))] if folds and (rt.uniform() < 0.7 or not st) else []
            own = bool(rt.uniform() < 0.5)
            qs = [] if own else [HIST_QS[i] for i in rt.permutation(len(HIST_QS))[:int(rt.integers(0, 4))]]
            zonal.append(dict(zones=zones, external=external, stats=st, hists=hs, own=own, qs=qs,
                              max_zones=int(rt.choice([1 << 22, 1 << 22, 1 << 22, 3, 40]))))
    plan["zonal"] = zonal
    acc["labels"] = labels
    new = [dict(op="read_acc") for _ in range(int(rt.integers(1, 3)))]
    if trees or zonal:
        new += [dict(op="tables") for _ in range(int(rt.integers(1, 4)))]
    for e, sets in enumerate(labels):
        new += [dict(op="set_zones", entry=e, labels=k) for k in range(len(sets))]
    new = [new[i] for i in rt.permutation(len(new))]
    for e, sets in enumerate(labels):                            # (the set_zones of one grid keep their order)
        for k, o in enumerate(o for o in new if o["op"] == "set_zones" and o["entry"] == e):
            o["labels"] = k
    at = sorted(int(rt.integers(0, len(ops))) for _ in new)
    for k, (i, o) in enumerate(zip(at, new)):
        ops.insert(i + k, o)
    for i in range(1, len(ops)):                                 # a tables right behind an async ingest waits for nothing itself
        if ops[i]["op"] in ("read_acc", "tables") and ops[i - 1]["op"] == "ingest" and ops[i - 1]["how"].startswith("async"):
            ops[i - 1]["sync"] = ops[i - 1]["sync"] and bool(rt.uniform() < 0.5)


def build(seed):
    poly_seed = seed if seed >= POLY_SEED_BASE else None
    if poly_seed is not None:                                    # a polygon case: the accumulator case of this seed, then _poly_pass
        seed = seed - POLY_SEED_BASE + ACC_SEED_BASE
    rng = np.random.default_rng(91000 + seed)
    # How the sequence opens.  "union": what a row-block shard does -- one sparse cloud, the other ranks' flags merged in, finalize.
    # "overlay": a checkpoint of an earlier pipeline loaded over the first ingest of a new one.  "hot": the hot spot as the first
    # ingest of an in-core pipeline that is offered the bands, a blocking finalize behind it.  Else: anything.
    opening = str(rng.choice(["any", "union", "overlay", "hot"], p=[0.62, 0.14, 0.14, 0.10]))
    big = bool(rng.uniform() < 0.1)
    if big:
        W, H = 520, 512                                          # write_cog's rule yields a level only from 512 cells a side
    else:
        W, H = int(rng.integers(33, 301)), int(rng.integers(33, 261))
        if rng.uniform() < 0.3:
            W = max(36, W - W % 4)
    cs = float(rng.choice([0.5, 1.0, 2.0]))
    min_x, min_y = float(rng.integers(1, 40)) * cs * float(rng.choice([-1.0, 1.0])), float(rng.integers(1, 40)) * cs
    flavour = _draw_flavour(rng)
    if opening == "hot":
        W, flavour = max(36, W - W % 4), dict(flavour, ooc=False)
    g = dict(W=W, H=H, cs=cs, min_x=min_x, min_y=min_y, max_x=min_x + W * cs, max_y=min_y + H * cs,
             tw=int(rng.choice([16, 32, 64, 4096])), th=int(rng.choice([16, 48, 64, 4096])))
    if flavour["ooc"] and H <= g["th"]:                          # out of core: at least two rows of reference tiles
        g["th"] = 16

    # reductions
    specs = []
    wide = bool(rng.uniform() < 0.15)
    if wide:                                                     # one group with more than 8 outputs
        specs = [dict(type=str(rng.choice(TYPES[:5])), ch="a") for _ in range(int(rng.integers(9, 11)))]
    for _ in range(int(rng.integers(0 if wide else 1, 11 - len(specs)))):
        specs.append(dict(type=str(rng.choice(TYPES, p=[0.15, 0.15, 0.15, 0.15, 0.22, 0.18])), ch=str(rng.choice(["a", "b"]))))
    order = rng.permutation(len(specs))
    specs = [specs[i] for i in order]
    groups = groups_of(specs)

    filt = None
    if rng.uniform() < 0.4:
        op = str(rng.choice(OPS8))
        filt = dict(op=op, value=float(rng.integers(1, 3)), set=[float(v) for v in rng.choice(4, int(rng.integers(1, 4)), replace=False)])

    plan = _draw_plan(rng, specs, flavour["ooc"], big)
    fwfi = bool(rng.uniform() < 0.8)
    path = int(rng.choice([0, 1, 2], p=[0.25, 0.15, 0.6]))

    # the sequence
    n_ops = int(rng.integers(4, 13))
    writable = [i for i, s in enumerate(specs) if s["type"] in ("Sum", "Count", "Average")]
    ops, n_ingest, cur_flavour, checkpoints = [], 0, flavour, []

    def tiles(k):
        tx, ty = -(-W // g["tw"]), -(-H // g["th"])
        return [(int(rng.integers(0, ty)), int(rng.integers(0, tx))) for _ in range(k)]

    def draw_ingest():
        how = str(rng.choice(["host", "device", "async_pinned", "async_device", "file"], p=[0.3, 0.25, 0.17, 0.17, 0.11]))
        return dict(op="ingest", how=how, sync=bool(rng.uniform() < 0.5), chunk_frac=float(rng.choice([0.13, 0.4, 1.0])))

    def draw_planes_write():
        r = int(rng.choice(writable))
        slot = int(rng.choice(PLANES_OF[specs[r]["type"]]))
        h, w = int(rng.integers(1, 21)), int(rng.integers(1, 21))
        r0, c0 = int(rng.integers(0, H - min(h, H) + 1)), int(rng.integers(0, W - min(w, W) + 1))
        if slot == 1:                                            # a Count plane: a few more points
            value = float(rng.integers(1, 4))
        elif specs[r]["ch"] == "b":                              # the sums of `b` are integers up to 2^23: so is the patch
            value = float(rng.integers(-PATCH_UNITS, PATCH_UNITS + 1))
        else:
            value = float(rng.integers(-PATCH_UNITS, PATCH_UNITS + 1)) / 8.0
        return dict(op="planes_write", group=specs[r]["group"], slot=slot, rect=(r0, c0, min(h, H), min(w, W)), value=value)

    if opening != "any":                                         # (as a shard runs: the option on, the path left to the engine or binned)
        fwfi, path = True, int(rng.choice([0, 2]))
    if opening == "union":
        ops += [draw_ingest(), dict(op="merge", extra=tiles(int(rng.integers(1, 3)))), dict(op="finalize", wait=bool(rng.uniform() < 0.6))]
    elif opening == "hot":
        ops += [dict(draw_ingest(), how=str(rng.choice(["host", "device", "async_pinned", "async_device"]))), dict(op="finalize", wait=True)]
    elif opening == "overlay":
        ops += [draw_ingest(), dict(op="checkpoint", then="fresh", plan=None, flavour=None), draw_ingest(), dict(op="reload", of=1),
                dict(op="finalize", wait=bool(rng.uniform() < 0.6))]
        checkpoints.append(1)
    elif rng.uniform() < 0.2:                                    # a pointer handed out before the first ingest
        ops.append(dict(op="flags", readonly=False, extra=tiles(int(rng.integers(0, 2)))))
    elif rng.uniform() < 0.1:
        ops.append(dict(op="planes_read"))
    n_ingest = sum(o["op"] == "ingest" for o in ops)
    n_ops = min(12, max(n_ops, len(ops) + 2))
    while len(ops) < n_ops - 1:
        prev = ops[-1]["op"] if ops else None
        fresh = prev == "checkpoint" and ops[-1]["then"] == "fresh"
        if n_ingest == 0 or fresh or (prev == "checkpoint" and rng.uniform() < 0.6):
            kind = "ingest"
        elif checkpoints and rng.uniform() < (0.6 if len(ops) > 1 and ops[-2]["op"] == "checkpoint" and ops[-2]["then"] == "fresh" else 0.06):
            kind = "reload"                                      # an earlier checkpoint (of any pipeline of the case) laid over the state
        elif prev == "ingest":                                   # what may come between an ingest and its finalize
            kind = str(rng.choice(["finalize", "ingest", "planes_read", "planes_write", "flags_ro", "flags_rw", "merge", "checkpoint"],
                                  p=[0.4, 0.1, 0.1, 0.1, 0.05, 0.05, 0.08, 0.12]))
        else:
            kind = str(rng.choice(["finalize", "ingest", "planes_read", "planes_write", "flags_ro", "flags_rw", "merge", "checkpoint"],
                                  p=[0.2, 0.4, 0.04, 0.07, 0.04, 0.04, 0.11, 0.1]))
        if kind == "ingest":
            ops.append(draw_ingest())
            n_ingest += 1
        elif kind == "finalize":
            ops.append(dict(op="finalize", wait=bool(rng.uniform() < 0.6)))
        elif kind == "planes_write" and writable:
            ops.append(draw_planes_write())
        elif kind in ("planes_read", "planes_write"):
            ops.append(dict(op="planes_read"))
        elif kind in ("flags_ro", "flags_rw"):
            ops.append(dict(op="flags", readonly=kind == "flags_ro", extra=[] if kind == "flags_ro" else tiles(int(rng.integers(0, 2)))))
        elif kind == "merge":
            ops.append(dict(op="merge", extra=tiles(int(rng.integers(1, 3)))))
        elif kind == "reload":
            ops.append(dict(op="reload", of=int(checkpoints[-1] if rng.uniform() < 0.7 else rng.choice(checkpoints))))
        else:
            then = str(rng.choice(["go_on", "resume", "load", "fresh"], p=[0.25, 0.32, 0.25, 0.18]))
            o = dict(op="checkpoint", then=then, plan=None, flavour=None)
            if then != "go_on":                                  # the new pipeline: maybe another flavour, maybe another plan
                if rng.uniform() < 0.4:
                    o["flavour"] = dict(cur_flavour, ooc=not cur_flavour["ooc"] and H > g["th"])
                    cur_flavour = o["flavour"]
                if rng.uniform() < 0.6:
                    o["plan"] = _draw_plan(rng, specs, cur_flavour["ooc"], big)
            checkpoints.append(len(ops))
            ops.append(o)
    ops.append(dict(op="finalize", wait=bool(rng.uniform() < 0.6)))

    # clouds: one per ingest, thinned where a cell's sums would leave the exact range
    hot = bool(rng.uniform() < 0.12)
    shapes = [str(rng.choice(["all", "strip", "cluster", "outside", "empty"], p=[0.45, 0.2, 0.2, 0.08, 0.07])) for _ in range(n_ingest)]
    if shapes[0] in ("outside", "empty") and rng.uniform() < 0.7:
        shapes[0] = "all"
    if opening == "union":
        shapes[0] = str(rng.choice(["strip", "cluster"]))
    if opening == "hot":
        shapes[0] = "hot"
    if hot:
        shapes[int(rng.integers(0, n_ingest))] = "hot"
    clouds = []
    units_a, units_b = np.zeros(W * H), np.zeros(W * H)
    for shape in shapes:
        c = _draw_cloud(rng, g, shape, filt)
        while True:
            cell = cells_of(g, c["x"], c["y"])
            m = cell >= 0
            ua = units_a + np.bincount(cell[m], np.abs(c["a"][m].astype(np.float64)) * 8.0, W * H)
            ub = units_b + np.bincount(cell[m], c["b"][m].astype(np.float64), W * H)
            if max(ua.max(), ub.max()) < EXACT_UNITS:
                break
            _thin(c, np.arange(len(c["x"])) % 2 == 0)            # (a cloud that would break the condition is thinned)
        units_a, units_b = ua, ub
        clouds.append(c)
    # the condition on the inputs: every sum of every cell is exact in binary32, in any order -- the plane patches included
    # (units of 1/8 on an `a` plane, of 1 on a `b` plane, like the clouds'; a Count never exceeds the points of a cell)
    patched = PATCH_UNITS * sum(o["op"] == "planes_write" for o in ops)
    assert units_a.max() + patched < 1 << 24 and units_b.max() + patched < 1 << 24
    line = LINE_SEED_BASE <= seed < ACC_SEED_BASE
    acc = None
    if seed >= ACC_SEED_BASE:
        # an accumulator case: in core, no line pass; everything else of it drawn last and from generators of its own
        flavour = dict(flavour, ooc=False)
        groups, acc = _acc_pass(seed, g, specs, ops, clouds, filt, plan)
        assert point_units(g, clouds).max() + PATCH_UNITS * sum(o["op"] == "planes_write" for o in ops) < 1 << 24
    if line:
        # (it replaces clouds, thins others and adds plane writes: the Point condition again, on the clouds as they are now --
        # _line_pass holds the replaced clouds to it as it holds them to the Line condition)
        groups = _line_pass(seed, g, specs, ops, clouds, filt)
        assert point_units(g, clouds).max() + PATCH_UNITS * sum(o["op"] == "planes_write" for o in ops) < 1 << 24
    k = 0
    for o in ops:
        if o["op"] == "ingest":
            o["cloud"] = k
            if len(clouds[k]["x"]) == 0 and o["how"] != "host":   # (an empty cloud has no file and no device copy)
                o["how"] = "host"
            k += 1

    case = dict(seed=seed, grid=g, specs=specs, groups=groups, filt=filt, plan=plan, flavour=flavour, fwfi=fwfi, path=path,
                ops=ops, clouds=clouds, big=big, wide=wide, line=line, acc=acc)
    first = clouds[next(o for o in ops if o["op"] == "ingest")["cloud"]]
    offered = _first_ingest_is_offered(case)
    case["marked"] = offered and first["shape"] != "hot"
    # ... or is offered them and splits a bin, so that the device's done word says no: the blocking finalize behind it reads 0
    case["split_first"] = offered and opening == "hot" and hot_records(case, first) > SPLIT_RECORDS
    if acc is not None:                                          # (the marks are about the Point groups' stored bands: the last scatter of an
        case["marked"] = case["split_first"] = False             # accumulator case's ingest is an accumulator's, and a filtered group is not offered)
    # the terrain bands of every plan, last and from generators of their own: no draw above moves, a seed stays the case it was
    # (tests/golden/sequence_fuzz_cases.json).  k = 0: the opening plan; k = index + 1: the plan of the checkpoint at ops[index]
    plan["terrain"] = _draw_terrain(np.random.default_rng((93000, seed, 0)), specs, plan, acc_terrain_sources(acc) if acc else ())
    if acc is not None:
        _acc_tables(seed, case)
    for i, o in enumerate(ops):
        if o["op"] == "checkpoint" and o["plan"] is not None:
            o["plan"]["terrain"] = _draw_terrain(np.random.default_rng((93000, seed, i + 1)), specs, o["plan"])
    case["poly"] = None
    if poly_seed is not None:
        case["seed"] = poly_seed
        _poly_pass(poly_seed, case)
    return case


def case_digest(case):
    """SHA-256 of what a seed means apart from the terrain lists: grid, specs (a line case: with their glyphs), filter, flavour,
    fwfi, path, the opening plan and the ops (with their plans) as sorted-key JSON, every cloud array's dtype and bytes (a line
    case: `dir` and `hl` too), `marked` and `split_first`.  tests/golden/sequence_fuzz_cases.json holds it for the 40 seeds that
    were the suite before terrain was drawn, and for LINE_SEEDS."""
    import hashlib
    import json

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(w) for k, w in v.items() if k != "terrain"}
        if type(v) is float and not np.isfinite(v):              # (an accumulator case: max_gap = +Inf)
            return repr(v)
        if isinstance(v, (list, tuple)):
            return [plain(w) for w in v]
        assert v is None or type(v) in (bool, int, float, str), type(v)
        return v

    h = hashlib.sha256()
    head = {k: plain(case[k]) for k in ("grid", "specs", "filt", "flavour", "fwfi", "path", "plan", "ops", "marked", "split_first")}
    if case.get("acc") is not None:                              # an accumulator case: the lists, and the plan's terrain after all
        head["acc"] = plain(case["acc"])                          # (its sources are part of what the case is for)
        head["terrain"] = plain(case["plan"]["terrain"])
    if case.get("poly") is not None:                             # a polygon case: the sets' options, the uses, the entries (the new ops
        po = case["poly"]                                        # are in `ops`, `lab` is a cloud key); the vertex bits below
        head["poly"] = plain({k: v for k, v in po.items() if k not in ("sets", "zone_sets")})
        head["poly_sets"] = plain([[st["opts"] for st in sets] for sets in po["sets"]] + [st["opts"] for st in po["zone_sets"]])
    h.update(json.dumps(head, sort_keys=True, allow_nan=False).encode())
    if case.get("poly") is not None:
        for st in [st for sets in case["poly"]["sets"] for st in sets] + case["poly"]["zone_sets"]:
            pl = st["polys"]
            for a in (pl.coords, pl.ring_offsets, pl.polygon_offsets) + (() if pl.values is None else (pl.values,)):
                h.update(f"{a.dtype.str}:{a.shape}".encode())
                h.update(np.ascontiguousarray(a).tobytes())
    for c in case["clouds"]:
        h.update(c["shape"].encode())
        for k in cloud_keys(c):
            a = np.ascontiguousarray(c[k])
            h.update(f"{k}:{a.dtype.str}:{a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def keep_mask(filt, cls):
    if filt is None:
        return np.ones(len(cls), bool)
    v, op = np.float32(filt["value"]), filt["op"]
    if op in ("InSet", "NotInSet"):
        inside = np.isin(cls, np.array(filt["set"], np.float32))
        return inside if op == "InSet" else ~inside
    return {"Equal": cls == v, "NotEqual": cls != v, "Less": cls < v, "LessEqual": cls <= v, "Greater": cls > v,
            "GreaterEqual": cls >= v}[op]


def _first_ingest_is_offered(case):
    """The first ingest is certain to be offered the bands and (case["marked"]: unless it is the hot spot) to store them -- Pipeline::Impl::offer_bands and the engine's
    finalize_taken (binned_point: define_all and fused): in core, the option on, no pointer handed out and no state imported
    before it (it is the first op, or only a read-only flag pointer precedes it), one cloud in one scatter that the filter
    leaves points of, the binned path taken (forced, or chosen by the engine: cells <= 16 n), whole float4 groups
    (W % 4 == 0), and a non-select group of at most 8 outputs."""
    g, ops = case["grid"], case["ops"]
    first = next(i for i, o in enumerate(ops) if o["op"] == "ingest")
    if any(not (o["op"] == "flags" and o["readonly"]) for o in ops[:first]):
        return False
    o, c = ops[first], case["clouds"][ops[first]["cloud"]]
    n = len(c["x"])
    if case["flavour"]["ooc"] or not case["fwfi"] or o["how"] == "file" or n == 0 or g["W"] % 4:
        return False
    if not keep_mask(case["filt"], c["cls"]).any():
        return False
    if not (case["path"] == 2 or (case["path"] == 0 and n * 16 >= g["W"] * g["H"])):
        return False
    return any(point_accumulation(gr) and len(gr["outs"]) <= MAX_FINALIZE_OUTPUTS for gr in case["groups"])


def point_accumulation(gr):
    """A group that offer_bands may offer the bands of: not MostRecent, and the Point glyph (it refuses glyph groups)."""
    return not gr["select"] and gr["glyph"] is None


def defers_for_sure(case):
    """... and leaves a plane in its band: an own-plane reduction (Sum, Count, Max, Min) is an output of such a group."""
    return (case["marked"] or case["split_first"]) and any(point_accumulation(gr) and len(gr["outs"]) <= MAX_FINALIZE_OUTPUTS and
                                  any(case["specs"][r]["type"] in ("Sum", "Count", "Max", "Min") for r in gr["outs"])
                                  for gr in case["groups"])


def segments(case):
    """The sequence cut at every checkpoint that a new pipeline resumes from: [(plan, flavour, ops, resumed plan differs,
    the pipeline took the checkpoint (resume or load) under another terrain list)]."""
    out, plan, flavour, cur, differs, terrain_differs = [], case["plan"], case["flavour"], [], False, False
    for o in case["ops"]:
        cur.append(o)
        if o["op"] == "checkpoint" and o["then"] != "go_on":
            out.append((plan, flavour, cur, differs, terrain_differs))
            differs = o["plan"] is not None and any(o["plan"][k] != plan[k] for k in ("fill", "ground", "loc"))
            terrain_differs = o["plan"] is not None and o["then"] in ("resume", "load") and o["plan"]["terrain"] != plan["terrain"]
            plan, flavour, cur = o["plan"] or plan, o["flavour"] or flavour, []
    out.append((plan, flavour, cur, differs, terrain_differs))
    return out


def situations(case):
    """Which of the situations the fuzz is for occur in a case (tests/test_sequence_fuzz_host.py counts them over the seeds).
    Only what runs on the HIP engine counts: pointer ops in in-core segments, a hot spot that is binned."""
    if case.get("poly") is not None:                             # (a polygon case has situations of its own)
        return poly_situations(case)
    if case.get("acc") is not None:                              # (an accumulator case has situations of its own)
        return acc_situations(case)
    found = set()
    types = [s["type"] for s in case["specs"]]
    real = lambda o: o["op"] == "ingest" and len(case["clouds"][o["cloud"]]["x"]) > 0
    if case["split_first"]:
        found.add("a split bin in the offered first ingest")
    if any(len(gr["outs"]) > MAX_FINALIZE_OUTPUTS for gr in case["groups"]):
        found.add("more than 8 outputs in a group")
    stored = [point_accumulation(gr) and len(gr["outs"]) <= MAX_FINALIZE_OUTPUTS for gr in case["groups"]]
    names = [band_name(i, sp) for i, sp in enumerate(case["specs"])]
    for s, (plan, flavour, ops, differs, terrain_differs) in enumerate(segments(case)):
        ingests = finalizes = 0
        terrain = plan["terrain"]
        of_specs = [case["specs"][names.index(t["source"])] for t in terrain if t["source"] in names]
        disturbed = False                                        # the state was changed from outside since this pipeline's last finalize
        for i, o in enumerate(ops):
            prev = ops[i - 1] if i else None
            if o["op"] == "finalize" and terrain:
                if case["marked"] and s == 0 and ingests == 1 and prev is not None and real(prev) and any(stored[sp["group"]] for sp in of_specs):
                    found.add("terrain of a band that the first ingest stored, finalize right behind it")
                if plan["fill"] > 0 and any(sp["type"] in FILL_TYPES for sp in of_specs):
                    found.add("terrain of a filled band")
                if plan["fill"] > 0 and any(t["source"] in ("dtm", "hag") for t in terrain):
                    found.add("terrain of dtm or hag, filled")
                for l in terrain_launches(terrain):
                    hs = [m for m in l if terrain[m]["product"] == "hillshade"]
                    light = lambda m: (terrain[m]["azimuth"], terrain[m]["altitude"])
                    # (a light that is neither the default nor the first entry's: taking either instead shows)
                    if len(l) >= 2 and hs and hs[0] != l[0] and light(hs[0]) not in (TERRAIN_LIGHTS[0], light(l[0])):
                        found.add("a launch whose hillshade entry is not its first, light not the default")
                if flavour["ooc"]:
                    found.add("terrain out of core")
                elif plan["loc"] == "Device":
                    found.add("terrain with a Device result")
                if case["big"] and plan["out"] and plan["cog"]:
                    found.add("terrain in a GeoTIFF with a write_cog level")
                if finalizes and disturbed:
                    found.add("terrain finalized again after a plane write, merge_touched or load_state")
                if any(len(case["groups"][sp["group"]]["outs"]) > MAX_FINALIZE_OUTPUTS for sp in of_specs):
                    found.add("terrain source in a group of more than 8 outputs")
            if o["op"] == "finalize":
                if terrain_differs:                              # (bands added, dropped or changed: an empty list counts)
                    found.add("resume or load under another terrain list")
                disturbed = False
            elif o["op"] in ("planes_write", "merge") and not flavour["ooc"] or o["op"] == "reload" and ingests:
                disturbed = True
            if o["op"] == "finalize":
                if case["fwfi"] and ingests == 1 and prev is not None and real(prev):
                    found.add("finalize right after the only ingest, finalize_with_first_ingest on")
                if plan["ground"] and plan["fill"] > 0 and ingests >= 2 and finalizes >= 1 and prev is not None and real(prev):
                    found.add("ground + fill + a second ingest")
                if case["big"] and plan["out"] and plan["cog"]:
                    found.add("write_cog level")
                finalizes += 1
            elif real(o):
                # (the binned path of an in-core pipeline: more than 2^17 records past the filter in one LDS tile)
                if not flavour["ooc"] and case["path"] != 1 and hot_records(case, case["clouds"][o["cloud"]]) > SPLIT_RECORDS:
                    found.add("hot spot")
                if finalizes:
                    found.add("ingest after a finalize")
                ingests += 1
            elif o["op"] in ("planes_read", "planes_write", "flags", "merge") and flavour["ooc"]:
                pass                                             # (out of core hands out no pointers: the runner drops the op)
            elif o["op"] in ("planes_read", "planes_write"):
                if o["op"] == "planes_write":
                    found.add("plane write")
                if prev is not None and real(prev) and any(q["op"] == "finalize" for q in ops[i:]):
                    found.add("state_planes() between an ingest and its finalize")
            elif o["op"] == "flags" and not o["readonly"] and s == 0 and ingests == 0:
                found.add("writable flag pointer before the first ingest")
            elif o["op"] == "merge" and finalizes:
                found.add("merge_touched after a finalize")
            elif o["op"] == "checkpoint" and ingests == 1:
                found.add("checkpoint after a single ingest")
            elif o["op"] == "reload" and ingests and any(q["op"] == "finalize" for q in ops[i:]):
                found.add("load_state over a state that was ingested into")
        if differs:
            found.add("resume under a different finalize plan")
        if flavour["ooc"] and any(o["op"] == "finalize" for o in ops):
            if "MostRecent" in types:
                found.add("out of core with MostRecent")
            if plan["ground"] or plan["fill"] > 0:
                found.add("out of core with ground or fill")
    return found | (line_situations(case) if case["line"] else set())


def line_binned(case, o):
    """The Line scatters of this ingest into an in-core pipeline go through the tile kernels as ONE scatter: the binned path
    forced, or chosen by the engine (binned_glyph_supported: 64 n >= cells).  A file ingest scatters chunk by chunk."""
    n, g = len(case["clouds"][o["cloud"]]["x"]), case["grid"]
    return o["how"] != "file" and (case["path"] == 2 or (case["path"] == 0 and n * 64 >= g["W"] * g["H"]))


def line_situations(case):
    """The LINE_SITUATIONS that occur in a line case, from the case alone (as situations(): only what runs on the HIP engine)."""
    found = set()
    g, specs, groups = case["grid"], case["specs"], case["groups"]
    lines = [gr for gr in groups if gr["glyph"] is not None]
    names = [band_name(i, s) for i, s in enumerate(specs)]
    line_bands = [names[i] for i, s in enumerate(specs) if "glyph" in s]
    if any(gr["glyph"] is None and gr["ch"] == lg["ch"] for gr in groups for lg in lines):
        found.add("a Line group and a Point group on one value channel")
    if any(a["ch"] == b["ch"] and sum(a["glyph"][k] != b["glyph"][k] for k in a["glyph"]) == 1 for a in lines for b in lines):
        found.add("two Line groups on one channel that differ in one glyph parameter")
    for lg in lines:
        found.add(f"Line mask {sum(1 << p for p in lg['slots'])}")
    if any(s["type"] == "WeightedAverage" and "glyph" not in s for s in specs):
        found.add("a WeightedAverage Point reduction")
    per_point = any(lg["glyph"]["hl_ch"] for lg in lines)
    segs = segments(case)
    ever = False                                                 # a Line state that holds something
    for s, (plan, flavour, ops, differs, terrain_differs) in enumerate(segs):
        ingests = finalizes = 0
        undefined, ooc = s == 0, flavour["ooc"]
        written = set()
        for i, o in enumerate(ops):
            prev = ops[i - 1] if i else None
            c = case["clouds"][o["cloud"]] if o["op"] == "ingest" else None
            inside = c is not None and len(c["x"]) > 0 and cells_of(g, c["x"], c["y"]) >= 0
            kept = inside & keep_mask(case["filt"], c["cls"]) if c is not None and len(c["x"]) else np.zeros(0, bool)
            if o["op"] == "ingest" and not kept.any():
                continue                                         # (nothing is scattered)
            if o["op"] == "ingest":
                binned = not ooc and line_binned(case, o)
                if per_point and (c["hl"][kept] < 0).any() and (c["hl"][kept] == 0).any():
                    found.add("a per-point hl with negative and zero entries")
                if (np.abs(c["dir"][kept]) > 64).any():
                    found.add("directions beyond +-64 rad")
                if per_point and binned and (c["hl"][kept] >= np.float32(LINE_LONG_CELLS * g["cs"])).any():
                    found.add("a segment beyond the record range")
                if undefined and not ooc and binned:
                    found.add("a first Line ingest into undefined planes, binned")
                elif undefined and not ooc and o["how"] != "file" and not line_binned(case, o):
                    found.add("a first Line ingest into undefined planes, direct")
                if finalizes:
                    found.add("a Line ingest after a finalize")
                if ooc and c["shape"] == "cluster" and any(q["op"] == "finalize" for q in ops[i:]):
                    found.add("out of core with a Line group and a cloud clustered on a reference-tile corner")
                if case["filt"] and kept.sum() < inside.sum():
                    found.add("a filter that removes points of a Line cloud")
                for lg in lines if binned else []:
                    if line_tile_records(case, c, lg).sum() > LINE_ITEM_RECORDS:
                        found.add("a hot Line tile")
                    load = line_list_load(case, c, lg)
                    # (a segment whose clipped part is empty is not listed: at most a few in a hundred, a quarter is allowed for)
                    if load and load[3] <= LINE_ITEM_RECORDS and load[0] * 4 >= load[2] * 5:
                        found.add("late-large values in a packed item: the list overflown")
                    elif load and load[3] <= LINE_ITEM_RECORDS and load[0] >= 8 and load[1] <= load[2]:
                        found.add("late-large values in a packed item: the list used")
                ingests, ever = ingests + 1, True
            elif o["op"] == "finalize":
                if case["marked"] and s == 0 and ingests == 1 and prev is not None and prev["op"] == "ingest":
                    found.add("a Line group next to a Point group whose bands the first ingest stored, finalize right behind it")
                if (plan["fill"] > 0 and any("glyph" in sp and sp["type"] in FILL_TYPES for sp in specs)) or \
                        any(t["source"] in line_bands for t in plan["terrain"]):
                    found.add("fill or terrain on a Line band")
                found |= written
                written = set()
                finalizes += 1
            elif o["op"] == "planes_write" and not ooc and groups[o["group"]]["glyph"] is not None:
                written.add(f"a plane write into a Line group's {'weight' if o['slot'] else 'sum'} plane, then a finalize")
            elif o["op"] == "checkpoint" and o["then"] in ("resume", "load") and o["flavour"] is not None and o["flavour"]["ooc"] != ooc and \
                    ever and any(q["op"] == "finalize" for q in segs[s + 1][2]):
                found.add("a Line checkpoint of an out-of-core pipeline taken in core" if ooc else "a Line checkpoint of an in-core pipeline taken out of core")
            elif o["op"] == "reload" and ingests and any(q["op"] == "finalize" for q in ops[i:]):
                found.add("load_state over a Line state that was ingested into")
            undefined = False
    return found


LINE_SITUATIONS = ("a Line group and a Point group on one value channel", "two Line groups on one channel that differ in one glyph parameter",
                   "Line mask 1", "Line mask 2", "Line mask 3", "a per-point hl with negative and zero entries",
                   "directions beyond +-64 rad", "a segment beyond the record range",
                   "a Line group next to a Point group whose bands the first ingest stored, finalize right behind it",
                   "a first Line ingest into undefined planes, binned", "a first Line ingest into undefined planes, direct",
                   "a Line ingest after a finalize", "a plane write into a Line group's sum plane, then a finalize",
                   "a plane write into a Line group's weight plane, then a finalize",
                   "a Line checkpoint of an in-core pipeline taken out of core", "a Line checkpoint of an out-of-core pipeline taken in core",
                   "load_state over a Line state that was ingested into",
                   "out of core with a Line group and a cloud clustered on a reference-tile corner", "a hot Line tile",
                   "late-large values in a packed item: the list used", "late-large values in a packed item: the list overflown",
                   "a filter that removes points of a Line cloud", "a WeightedAverage Point reduction", "fill or terrain on a Line band")
# The line cases of the suite: the smallest list of seeds >= LINE_SEED_BASE in which every entry above occurs three times
# (greedy cover of 2000..2399, cheaper cases first; tests/test_sequence_fuzz_host.py counts).  A failing seed of a soak joins it.
LINE_SEEDS = [
    2009,   # mask 1 beside a Point group on its channel; an out-of-core checkpoint taken in core
    2056,   # 520 x 512: two glyphs on one channel, masks 1 and 3, a hot Line tile, a segment of 40 000 cells, a filter
    2071,   # out of core first, then in core: a cluster on a tile corner, a write into a weight plane
    2113,   # 520 x 512: Line groups beside stored Point bands, the finalize right behind the first ingest; masks 2 and 3
    2133,   # a first Line ingest on the direct path; writes into the sum and the weight plane of a mask-3 group
    2136,   # a packed item whose list overflows and one whose list is used; stored Point bands beside the Line groups
    2213,   # in core, then resumed out of core; stored Point bands beside masks 1 and 3
    2251,   # a direct first ingest; the checkpoint taken out of core, a cluster on a tile corner there
    2272,   # mask 1 alone: a direct first ingest, a write into its sum plane
    2275,   # two glyphs on one channel; load_state over an ingested Line state; in core to out of core, a cluster there
    2297,   # a packed item whose list overflows, ingested after a finalize; fill on a WeightedAverage Line band
    2328,   # two glyphs on one channel, both late-large clouds: the list overflown and the list used
    2331,   # mask 2; in core to out of core and back
    2344,   # a hot Line tile, the list used, writes into both planes, load_state over the state
    2385,   # masks 2 and 3: a hot Line tile, the list used, a write into a weight plane
]

ACC_SITUATIONS = ("two entries sharing a class", "an entry whose filter empties a cloud that the pipeline filter keeps",
                  "direct and binned scatters of one accumulator in one sequence", "a split bin in an accumulator tile",
                  "ingest_file in chunks with a surface channel", "an async ingest followed by read_acc without a synchronize in between",
                  "a DTM from an extremes band with fill > 0", "terrain of a Mean band", "trees of a Max-of-hag band",
                  "trees of a filled band", "zonal by tree_id with a Device result", "zonal by tree_id with a Host result",
                  "zonal by an external grid set after the finalize", "tables after an ingest (refused)",
                  "tables after a plane read or write", "tables after merge_touched",
                  "a second finalize with nothing new followed by tables", "a refused save_state between two ingests",
                  "max_zones exceeded", "no accumulator band sourced anywhere, trees and zonal present",
                  "a cloud that the pipeline filter empties", "tables after a cloud that the pipeline filter empties (still valid)")


def acc_situations(case):
    """The ACC_SITUATIONS that occur in an accumulator case, from the case alone.  "Binned" is the engine's own rule for a
    cloud of n points (forced, or cells <= 16 n); a split bin is counted only where more than ACC_ITEM_RECORDS accepted records
    lie in the first 128 x 8 cells, which every accumulator's first tile contains."""
    found = set()
    g, acc, plan, ops, specs = case["grid"], case["acc"], case["plan"], case["ops"], case["specs"]
    cells = g["W"] * g["H"]
    entries = acc_entries(acc)
    keys = [filter_key(e["filt"]) for e in entries if e["filt"]]
    if len(set(keys)) < len(keys) or set(keys) & {filter_key(s["filt"]) for s in specs if s["filt"]}:
        found.add("two entries sharing a class")
    kinds = {n: kind for n, kind, _, _ in acc_bands(acc)}
    by_name = {band_name(i, s): s for i, s in enumerate(specs)}
    filled = lambda n: n in ("dtm", "hag") or (n in kinds and acc_filled(kinds[n])) or (n in by_name and by_name[n]["type"] in FILL_TYPES)
    trees, zonal = plan["trees"], plan["zonal"]
    sourced = [t["source"] for t in plan["terrain"]] + [t["source"] for t in trees] + (list(ground_names(specs, plan)) if plan["ground"] else [])
    if plan["ground"] and plan["fill"] > 0 and kinds.get(ground_names(specs, plan)[0]) == "extremes":
        found.add("a DTM from an extremes band with fill > 0")
    if any(kinds.get(t["source"]) == "mean" for t in plan["terrain"]):
        found.add("terrain of a Mean band")
    if any(t["source"] in by_name and by_name[t["source"]]["type"] == "Max" and by_name[t["source"]]["ch"] == "hag" for t in trees):
        found.add("trees of a Max-of-hag band")
    if plan["fill"] > 0 and any(filled(t["source"]) for t in trees):
        found.add("trees of a filled band")
    if any(not z["external"] for z in zonal):
        found.add(f"zonal by tree_id with a {plan['loc']} result")
    if trees and zonal and not any(n in kinds for n in sourced):
        found.add("no accumulator band sourced anywhere, trees and zonal present")
    externals = [z for z in zonal if z["external"]]
    for z, sets in zip(externals, acc["labels"]):
        lab = external_labels(g, sets[0])
        with np.errstate(all="ignore"):
            valid = np.isfinite(lab) & (lab >= 1) & (lab == np.floor(lab))
        if valid.any() and lab[valid].max() > z["max_zones"]:
            found.add("max_zones exceeded")
    finalized = fresh = False
    since = set()                                                # what happened since the last finalize
    paths = set()
    n_ingest = sum(o["op"] == "ingest" for o in ops)
    seen_ingests = 0
    for i, o in enumerate(ops):
        nxt = ops[i + 1] if i + 1 < len(ops) else None
        if o["op"] == "ingest":
            seen_ingests += 1
            c = case["clouds"][o["cloud"]]
            n = len(c["x"])
            keep = keep_mask(case["filt"], c["cls"])
            if not keep.any():                                   # (in.kept == 0: the ingest returns before any accumulator runs)
                if n:
                    found.add("a cloud that the pipeline filter empties")
                    since.add("filtered cloud")
                continue
            fresh = False
            since = set()
            chunk = max(1, int(n * o["chunk_frac"])) if o["how"] == "file" else n
            if o["how"] == "file" and chunk < n and acc["surfaces"]:
                found.add("ingest_file in chunks with a surface channel")
            if o["how"].startswith("async") and not o["sync"] and nxt is not None and nxt["op"] == "read_acc":
                found.add("an async ingest followed by read_acc without a synchronize in between")
            binned = case["path"] == 2 or (case["path"] == 0 and chunk * 16 >= cells)
            paths.add("binned" if binned else "direct")
            ch = surface_channels(acc, c)
            cell = cells_of(g, c["x"], c["y"])
            first = (cell >= 0) & (cell // g["W"] < ACC_HOT_H) & (cell % g["W"] < ACC_HOT_W)
            for e in entries:
                mine = keep & conj_mask(ch, e["filt"], n)
                if e["filt"] and not mine.any():
                    found.add("an entry whose filter empties a cloud that the pipeline filter keeps")
                if binned and o["how"] != "file" and (mine & first & ~np.isnan(ch[e["ch"]])).sum() > ACC_ITEM_RECORDS:
                    found.add("a split bin in an accumulator tile")
        elif o["op"] == "finalize":
            if fresh and (trees or zonal):                       # (the runner reads every table behind every finalize)
                found.add("a second finalize with nothing new followed by tables")
            finalized = fresh = True
            since = set()
        elif o["op"] in ("planes_read", "planes_write", "merge"):
            since.add(o["op"])
        elif o["op"] == "set_zones" and finalized and fresh:
            since.add("set_zones")
        elif o["op"] == "tables":
            if zonal and finalized and not fresh:
                found.add("tables after an ingest (refused)")
            if finalized and fresh and since & {"planes_read", "planes_write"}:
                found.add("tables after a plane read or write")
            if finalized and fresh and "merge" in since:
                found.add("tables after merge_touched")
            if zonal and finalized and fresh and "filtered cloud" in since:
                found.add("tables after a cloud that the pipeline filter empties (still valid)")
            if finalized and fresh and "set_zones" in since:
                found.add("zonal by an external grid set after the finalize")
        elif o["op"] == "checkpoint" and 0 < seen_ingests < n_ingest:
            found.add("a refused save_state between two ingests")
    if paths == {"direct", "binned"}:
        found.add("direct and binned scatters of one accumulator in one sequence")
    return found


# The accumulator cases of the suite: a greedy cover of 10000..10399 in which every entry above occurs four times, cheaper cases
# first (tests/test_sequence_fuzz_host.py asks for three).  A failing seed of a soak joins it.
ACC_SEEDS = [
    10003,  # Auto: direct and binned; trees of a Max-of-hag band; read_acc behind an async ingest that nobody waited for
    10054,  # tables after a plane write and after merge_touched; a second finalize with nothing new
    10055,  # a split accumulator bin; zonal by tree_id, Host result; no accumulator band sourced anywhere
    10059,  # an external grid set after the finalize, max_zones exceeded; tables after a plane write and a merge
    10067,  # ingest_file in chunks with a surface channel; trees of Max-of-hag; zonal by tree_id, Device result
    10078,  # chunks with a surface channel; terrain of a Mean band
    10111,  # chunks with a surface channel; zonal by tree_id, Device result; tables after a plane read
    10113,  # Auto: direct and binned; zonal by tree_id, Device result
    10133,  # an external grid set after the finalize; trees of Max-of-hag; tables after a plane write and a merge
    10190,  # a split bin, direct and binned, read_acc behind an unwaited async ingest, max_zones exceeded
    10204,  # a split bin; tables refused after an ingest; terrain of a Mean band; zones by tree_id and external
    10207,  # a DTM from an extremes band, filled
    10208,  # terrain of a Mean band; trees of Max-of-hag; zonal by tree_id, Host result
    10216,  # a DTM from an extremes band, filled
    10259,  # a DTM from an extremes band, filled
    10264,  # a DTM from an extremes band, filled; zonal by tree_id, Device result, refused after an ingest
    10288,  # Auto: direct and binned; chunks with a surface channel; max_zones exceeded
    10312,  # a split bin; zonal by tree_id, Host result
    10339,  # an external grid set after the finalize; tables after merge_touched; terrain of a Mean band
    10431,  # a cloud that the pipeline filter empties (in.kept == 0: no accumulator runs)
    11192,  # tables right behind such a cloud: still valid (the host engine used to refuse them); a split bin
    11258,  # a cloud that the pipeline filter empties; terrain of a Mean band; max_zones exceeded
    11790,  # tables behind a cloud that the pipeline filter empties, and refused behind one that it keeps
    11833,  # tables behind a cloud that the pipeline filter empties and after merge_touched; zonal by tree_id, Host result
    11581,  # soak: two filters that differ only in a field their op does not use are ONE class (the model's filter_key kept them apart)
]

SITUATIONS = ("finalize right after the only ingest, finalize_with_first_ingest on", "ingest after a finalize",
              "state_planes() between an ingest and its finalize", "plane write", "writable flag pointer before the first ingest",
              "merge_touched after a finalize", "checkpoint after a single ingest", "resume under a different finalize plan",
              "hot spot", "ground + fill + a second ingest", "write_cog level", "more than 8 outputs in a group",
              "out of core with MostRecent", "out of core with ground or fill", "load_state over a state that was ingested into",
              "a split bin in the offered first ingest")
TERRAIN_SITUATIONS = ("terrain of a band that the first ingest stored, finalize right behind it", "terrain of a filled band",
                      "terrain of dtm or hag, filled", "a launch whose hillshade entry is not its first, light not the default",
                      "terrain out of core", "resume or load under another terrain list",
                      "terrain in a GeoTIFF with a write_cog level",
                      "terrain finalized again after a plane write, merge_touched or load_state",
                      "terrain source in a group of more than 8 outputs", "terrain with a Device result")
SITUATIONS += TERRAIN_SITUATIONS


# ---- polygon cases ---------------------------------------------------------------------------------------------------------------
# A seed from POLY_SEED_BASE on is a polygon case: the accumulator case of seed - POLY_SEED_BASE + ACC_SEED_BASE, then -- last and
# from generators of their own, (97000, seed, k) -- polygon channels and their sets, their uses, point zonal entries, the ops
# that set and read them, and what the clouds need for them (k = 0 the lists, 1 the ops, 10 + i cloud i).
POLY_SEED_BASE = 20000
POLY_NAMES = ("plot", "stand", "clip")
POLY_BACKGROUNDS = (float("nan"), -1.0, 0.0)
POLY_MAX_EDGES = 400                       # of one set: the models walk every edge for every point and every row
PZ_MAX_ZONES = (3, 40, 4096)
PZ_ITEM = 1 << 16                          # the fold's item: a cloud with more kept points in one zone meets one long run
PZ_CHANNELS = ("z", "a", "b")


def grid_geom(g):
    import rasterize_common as RC
    return RC.Geom(g["W"], g["H"], min_x=g["min_x"], max_y=g["max_y"], csx=g["cs"], csy=-g["cs"])


def _draw_polys(rp, g, outside):
    """One polygon set in the grid's world coordinates, from rasterize_common's makers: a jittered partition over part of the
    grid, a donut over it, a rectangle half outside the grid (`outside`: for sure), a handful of overlapping n-gons, one of
    points_in_polygons_common.degenerate()'s area-less polygons; then values (or none), a background and an index size.
    -> dict(polys, opts)"""
    import points_in_polygons_common as PIP
    import rasterize_common as RC
    w, h = g["W"] * g["cs"], g["H"] * g["cs"]
    x0, y0 = g["min_x"], g["min_y"]
    polygons, kinds, rect = [], [], None
    if rp.uniform() < 0.7:
        ax, ay = x0 + w * rp.uniform(0.0, 0.3), y0 + h * rp.uniform(0.0, 0.3)
        polygons += RC.partition(ax, ay, ax + w * rp.uniform(0.3, 0.65), ay + h * rp.uniform(0.3, 0.65), int(rp.integers(1, 4)),
                                 int(rp.integers(1, 4)), seed=int(rp.integers(0, 1 << 30)), wiggle=2)
        kinds.append("partition")
    if rp.uniform() < 0.4:
        r = min(w, h) * rp.uniform(0.1, 0.3)
        polygons.append(RC.donut(x0 + w * rp.uniform(0.2, 0.8), y0 + h * rp.uniform(0.2, 0.8), r, r * rp.uniform(0.2, 0.7), n=12))
        kinds.append("donut")
    if rp.uniform() < 0.5:
        cx, cy = x0 + w * rp.uniform(0.2, 0.8), y0 + h * rp.uniform(0.2, 0.8)
        for _ in range(int(rp.integers(2, 6))):
            polygons.append([RC.ngon(cx + w * rp.uniform(-0.1, 0.1), cy + h * rp.uniform(-0.1, 0.1), min(w, h) * rp.uniform(0.05, 0.2),
                                     int(rp.integers(3, 10)), rp.uniform(0, 1))])
        kinds.append("ngons")
    if rp.uniform() < 0.4:
        d = PIP.degenerate()
        k = int(rp.integers(1, 5))                               # no ring; three collinear points; a sliver of no height; forth and back
        ox, oy, s = x0 + w * rp.uniform(0.1, 0.8), y0 + h * rp.uniform(0.1, 0.8), 3.0 * g["cs"]
        polygons.append([np.array([ox, oy]) + s * ring for ring in d.polygon(k)])
        kinds.append(f"degenerate{k}")
    if outside or not polygons or rp.uniform() < 0.5:            # half outside the grid, to the right of it or above it
        if rp.uniform() < 0.5:
            rect = (g["max_x"] - w * rp.uniform(0.05, 0.2), y0 + h * rp.uniform(0.1, 0.4), g["max_x"] + w * rp.uniform(0.05, 0.2), y0 + h * rp.uniform(0.5, 0.9))
        else:
            rect = (x0 + w * rp.uniform(0.1, 0.4), g["max_y"] - h * rp.uniform(0.05, 0.2), x0 + w * rp.uniform(0.5, 0.9), g["max_y"] + h * rp.uniform(0.05, 0.2))
        rect = tuple(float(v) for v in rect)
        polygons.append([RC.rect(*rect)])
        kinds.append("rect")
    order = rp.permutation(len(polygons))
    polygons = [polygons[i] for i in order]
    P = len(polygons)
    values = None
    if rp.uniform() < 0.6:                                       # whole numbers a little beyond P, maybe one that is no zone
        values = rp.integers(1, P + 4, P).astype(np.float32)
        if rp.uniform() < 0.3:
            values[int(rp.integers(0, P))] = np.float32(rp.choice([2.5, 0.0, -3.0]))
    polys = RC.Polys(polygons, values)
    assert len(polys.coords) <= POLY_MAX_EDGES, len(polys.coords)
    cols, rows = PIP.INDEX_SIZES[int(rp.integers(0, len(PIP.INDEX_SIZES)))]
    opts = dict(background=float(POLY_BACKGROUNDS[int(rp.integers(0, 3))]), index_cols=cols, index_rows=rows, kinds=kinds,
                rect=None if rect is None else list(rect))
    return dict(polys=polys, opts=opts)


def set_values(st):
    """The values a set's polygons carry."""
    pl = st["polys"]
    return [float(v) for v in (np.arange(1, pl.P + 1, dtype=np.float32) if pl.values is None else pl.values)]


def _poly_pred(rp, name, sets):
    """A predicate on a polygon channel that keeps some points and drops others under most sets."""
    vals = sorted({v for st in sets for v in set_values(st)})
    kind = int(rp.integers(0, 5))
    some = [float(v) for v in rp.choice(vals, min(len(vals), int(rp.integers(1, 4))), replace=False)]
    op, value = (("GreaterEqual", 1.0), ("Greater", 0.0), ("InSet", 0.0), ("NotInSet", 0.0), ("LessEqual", vals[len(vals) // 2]))[kind]
    return dict(ch=name, op=op, value=float(value), set=some)


def poly_channels(case, k, current):
    """The polygon channels of cloud k under the sets `current` (an index per channel): points_in_polygons_common.model at the
    cloud's x and y, with the set's background as float32 bits.  Kept with the case: the model and poly_situations share them."""
    import points_in_polygons_common as PIP
    po, c = case["poly"], case["clouds"][k]
    memo = case.setdefault("_poly_memo", {})
    out = {}
    for name, sets, j in zip(po["names"], po["sets"], current):
        if (k, name, j) not in memo:
            st = sets[j]
            memo[(k, name, j)] = PIP.model(st["polys"], c["x"], c["y"], np.float32(st["opts"]["background"])) if len(c["x"]) else np.zeros(0, np.float32)
        out[name] = memo[(k, name, j)]
    return out


def pipeline_keep(case, ch):
    """PipelineConfig::filter of a case over the channels of a cloud: the `cls` predicate AND a polygon case's clip predicates."""
    keep = keep_mask(case["filt"], ch["cls"])
    return keep & conj_mask(ch, (case.get("poly") or {}).get("clip"), len(keep))


def zones_of(labels):
    """The zone of every label by zonal's rule (polygonize_common.zones_of: a whole number in [1, 2^24], else 0), as int64."""
    import polygonize_common as PG
    return PG.zones_of(labels).astype(np.int64)


def _poly_pass(seed, case):
    """What makes a seed >= POLY_SEED_BASE a polygon case, on top of the accumulator case `case`: the channels, their sets and
    their uses and the point zonal entries here (k = 0), then _poly_ops (k = 1) and _poly_clouds (k = 2 and 10 + i).  It only
    appends: reductions behind the reductions, a histogram behind the histograms, zonal entries behind the zonal entries, so
    every band and entry the accumulator case names keeps its index; a filter it replaces regroups the specs as in _acc_pass,
    and a plane write follows its reduction."""
    rp = np.random.default_rng((97000, seed, 0))
    g, specs, acc, ops, clouds = case["grid"], case["specs"], case["acc"], case["ops"], case["clouds"]
    names = list(POLY_NAMES[:int(rp.integers(1, 4))])
    sets = [[_draw_polys(rp, g, k == 0) for _ in range(int(rp.integers(1, 3)))] for k in range(len(names))]
    snames = [sc["name"] for sc in acc["surfaces"]]
    # the uses of every channel, each drawn on its own
    clip, ppool = [], []
    for name, ss in zip(names, sets):
        pred = _poly_pred(rp, name, ss)
        if rp.uniform() < 0.3:
            clip.append(pred)
        pred = _poly_pred(rp, name, ss)
        if rp.uniform() < 0.6:                                   # into the pool: alone, or behind a predicate on `cls`
            f = [pred]
            if rp.uniform() < 0.4:
                f.insert(0, dict(ch="cls", op=str(rp.choice(OPS8)), value=float(rp.integers(0, 4)),
                                 set=[float(v) for v in rp.choice(4, int(rp.integers(1, 4)), replace=False)]))
            ppool.append(f)
    old_pool = []
    for e in acc_entries(acc) + specs:
        if e["filt"] and filter_key(e["filt"]) not in [filter_key(q) for q in old_pool]:
            old_pool.append(e["filt"])
    pool = old_pool + ppool
    pick = lambda p: pool[int(rp.integers(0, len(pool)))] if pool and rp.uniform() < p else []
    for o in ops:                                                # (plane writes follow their reduction when the filters regroup the specs)
        if o["op"] == "planes_write":
            o["spec"] = next(i for i, s in enumerate(specs) if s["group"] == o["group"] and o["slot"] in PLANES_OF[s["type"]]
                             and s["type"] in ("Sum", "Count", "Average"))
    for e in acc_entries(acc) + specs:                           # a polygon predicate in the filters of what the case had
        if ppool and rp.uniform() < 0.25:
            e["filt"] = ppool[int(rp.integers(0, len(ppool)))]
    max_bands = []
    for name, ss in zip(names, sets):
        if rp.uniform() < 0.6:                                   # the channel as a value: selections and counts only, like `z`
            t = str(rp.choice(["Max", "Max", "Min", "Count"]))
            filt = pick(1.0 if t == "Count" else 0.5)
            if t == "Count" and not filt:                        # (a Count only under a filter; a case without one takes a Max)
                t = "Max"
            specs.append(dict(type=t, ch=name, filt=filt))
            if t == "Max":
                max_bands.append(band_name(len(specs) - 1, specs[-1]))
        if rp.uniform() < 0.4 and len(acc["hist"]) < 4:          # ... and as a histogram's channel, over the plot numbers (create takes 4)
            top = max([1.0] + [max(set_values(st)) for st in ss])     # (a set of one polygon of value -3 spans nothing)
            bins = int(rp.choice([8, 37]))
            qs = [HIST_QS[i] for i in rp.permutation(len(HIST_QS))[:int(rp.integers(0, 3))]]
            acc["hist"].append(dict(ch=name, lo=-1.5, hi=float(top) + 0.5, bins=bins, qs=qs, filt=pick(0.4)))
    groups = groups_of(specs)
    case["groups"] = groups
    for o in ops:
        if o["op"] == "planes_write":
            o["group"] = specs[o.pop("spec")]["group"]
    # point zonal entries
    pz = []
    labels = list(names) + [sc["name"] for sc in acc["surfaces"] if sc["mode"] == 0] + ["cls", "lab"]
    for i in range(int(rp.integers(1, 4))):
        label = names[int(rp.integers(0, len(names)))] if rp.uniform() < 0.5 else labels[int(rp.integers(0, len(labels)))]
        max_zones = int(rp.choice(PZ_MAX_ZONES))
        chans = list(PZ_CHANNELS) + snames + [n for n in names if n != label]
        n_stats, n_hists = int(rp.integers(0, 3)), int(rp.integers(0, 3))
        if n_stats + n_hists == 0:
            n_stats, n_hists = (1, 0) if rp.uniform() < 0.5 else (0, 1)
        st, hs = [], []
        for ch in rp.choice(chans, n_stats, replace=False):      # (two specs of one channel would name a column twice)
            origin, res = STAT_STEPS[int(rp.integers(0, 3))]
            st.append(dict(ch=str(ch), origin=origin, res=res, ddof=int(rp.integers(0, 2)), filt=pick(0.5)))
        for ch in rp.choice(chans, n_hists, replace=False):
            lo, hi = HIST_RANGES[int(rp.integers(0, len(HIST_RANGES)))]
            bins = int(rp.choice(HIST_BINS))
            if max_zones > 40:                                   # (the Python-int rows walk every bin of every zone)
                bins = min(bins, ZONAL_MAX_BINS)
            qs = [HIST_QS[j] for j in rp.permutation(len(HIST_QS))[:int(rp.integers(0, 4))]]
            hs.append(dict(ch=str(ch), lo=lo, hi=hi, bins=bins, qs=qs, filt=pick(0.5)))
        pz.append(dict(label=label, max_zones=max_zones, stats=st, hists=hs))
    distinct = {filter_key(e["filt"]) for e in acc_entries(acc) + specs + [s for e in pz for s in e["stats"] + e["hists"]] if e["filt"]}
    assert len(distinct) <= 8 and sum(len(k) for k in distinct) + (1 if case["filt"] else 0) + len(clip) <= 32, (seed, len(distinct))
    case["poly"] = dict(names=names, sets=sets, clip=clip, pz=pz, zone_sets=[], max_bands=max_bands)
    _poly_ops(seed, case)
    _poly_clouds(seed, case)
    assert point_units(g, clouds).max() + PATCH_UNITS * sum(o["op"] == "planes_write" for o in ops) < 1 << 24
    assert sum(len(c["x"]) for c in clouds) < 1 << 22


def _poly_ops(seed, case):
    """The ops of a polygon case, INSERTED into the sequence ahead of its last finalize as _acc_tables inserts its own, and the
    zonal entries they need: a twin of a by-tree entry for the reburn chain, an external entry for polygon-burnt zones."""
    ro = np.random.default_rng((97000, seed, 1))
    po, plan, acc, ops, specs = case["poly"], case["plan"], case["acc"], case["ops"], case["specs"]
    g = case["grid"]
    zonal, trees = plan["zonal"], plan["trees"]
    new = [dict(op="set_polygons", channel=k, sync=bool(ro.uniform() < 0.5)) for k, ss in enumerate(po["sets"]) if len(ss) == 2]
    new += [dict(op="point_tables", counts=bool(ro.uniform() < 0.5), sync=bool(ro.uniform() < 0.5)) for _ in range(int(ro.integers(1, 5)))]
    # the reburn chain: a by-tree entry and an external twin with the same lists, burnt from polygonize(tree_id)
    for i, z in enumerate(list(zonal)):
        if not z["external"] and len(zonal) < 4 and ro.uniform() < 0.5:
            zonal.append(dict(z, zones=f"burn{i}", external=True, twin_of=i))
            new += [dict(op="reburn", zonal=len(zonal) - 1, band=z["zones"]) for _ in range(int(ro.integers(1, 3)))]
    # zones burnt from a polygon set: on an external entry the case has, or on one of its own
    externals = [i for i, z in enumerate(zonal) if z["external"] and "twin_of" not in z]
    folds = [i for i, h in enumerate(acc["hist"]) if h["bins"] <= ZONAL_MAX_BINS]
    if not externals and len(zonal) < 4 and (acc["stats"] or folds) and ro.uniform() < 0.6:
        st = [int(ro.integers(0, len(acc["stats"])))] if acc["stats"] else []
        hs = [int(ro.choice(folds))] if folds and (ro.uniform() < 0.5 or not st) else []
        zonal.append(dict(zones="zp", external=True, stats=st, hists=hs, own=True, qs=[], max_zones=int(ro.choice([1 << 22, 3, 40]))))
        externals = [len(zonal) - 1]
    for i in externals:
        if ro.uniform() < 0.7:
            po["zone_sets"].append(_draw_polys(ro, g, False))
            new.append(dict(op="set_zones_poly", zonal=i, poly=len(po["zone_sets"]) - 1))
    # outlines: of a tree-id band, of a Max band of a polygon channel, of a Max band of `z`, of no band at all
    cands = [f"t{i}_id" for i in range(len(trees))] + po["max_bands"] + \
            [band_name(i, s) for i, s in enumerate(specs) if s["type"] == "Max" and s["ch"] == "z"][:1] + ["nope"]
    new += [dict(op="polygonize", band=cands[int(ro.integers(0, len(cands)))]) for _ in range(int(ro.integers(1, 4)))]
    po["outlines"] = sorted({o["band"] for o in new if o["op"] in ("polygonize", "reburn")})
    new = [new[i] for i in ro.permutation(len(new))]
    first = next(i for i, o in enumerate(ops) if o["op"] == "ingest")
    at = []
    for o in new:                                                # a second set comes between ingests; everything else anywhere
        lo = first + 1 if o["op"] == "set_polygons" else 0
        asyncs = [i + 1 for i in range(lo, len(ops)) if ops[i]["op"] == "ingest" and ops[i]["how"].startswith("async") and i + 1 < len(ops)]
        if o["op"] == "set_polygons" and asyncs and ro.uniform() < 0.5:
            at.append(int(ro.choice(asyncs)))                    # right behind an async ingest
        else:
            at.append(int(ro.integers(min(lo, len(ops) - 1), len(ops))))
    order = np.argsort(at, kind="stable")
    for k, j in enumerate(order):
        ops.insert(at[j] + k, new[j])
    for i in range(1, len(ops)):                                 # right behind an async ingest they wait for nothing themselves
        if ops[i]["op"] in ("set_polygons", "point_tables") and ops[i - 1]["op"] == "ingest" and ops[i - 1]["how"].startswith("async"):
            ops[i - 1]["sync"] = ops[i - 1]["sync"] and ops[i]["sync"]


def poly_walk(case):
    """The ingests of a polygon case in order: [(op index, cloud index, the sets current then (an index per channel))]."""
    cur, out = [0] * len(case["poly"]["names"]), []
    for i, o in enumerate(case["ops"]):
        if o["op"] == "set_polygons":
            cur[o["channel"]] = 1
        elif o["op"] == "ingest":
            out.append((i, o["cloud"], tuple(cur)))
    return out


def cloud_channels(case, k, current):
    """Every channel of cloud k of a polygon case: its own, the surface channels, the polygon channels under `current`."""
    memo = case.setdefault("_surface_memo", {})
    if k not in memo:
        ch = surface_channels(case["acc"], case["clouds"][k])
        memo[k] = {n: ch[n] for n in (sc["name"] for sc in case["acc"]["surfaces"])}
    return dict(case["clouds"][k], **memo[k], **poly_channels(case, k, current))


def _poly_clouds(seed, case):
    """What the clouds of a polygon case need: maybe one with more than 2^16 kept points in one zone of entry 0, maybe one that
    the pipeline filter empties, `lab` on all where an entry folds by it, and in every cloud a share of points moved (x and y
    only) outside the grid and inside a polygon."""
    po, g, clouds, filt = case["poly"], case["grid"], case["clouds"], case["filt"]
    r0 = np.random.default_rng((97000, seed, 2))
    W, H, cs = g["W"], g["H"], g["cs"]
    walk = poly_walk(case)
    cur_of = {k: cur for _, k, cur in walk}
    free = [k for k, c in enumerate(clouds) if c["shape"] not in ("hot", "hot_acc") and k in cur_of]
    swap = {}
    for kind in ("hot_zone", "pipeline_emptied"):
        if free and r0.uniform() < 1 / 3:
            swap[free.pop(int(r0.integers(0, len(free))))] = kind
    e0 = po["pz"][0]
    lab_entries = [e for e in po["pz"] if e["label"] == "lab"]
    field = z_field(g, seed - POLY_SEED_BASE + ACC_SEED_BASE)
    cls4 = np.arange(4, dtype=np.float32)
    kept_cls = cls4[keep_mask(filt, cls4)]
    for k, c in enumerate(clouds):
        rc = np.random.default_rng((97000, seed, 10 + k))
        kind = swap.get(k)
        if kind == "hot_zone" and e0["label"] not in [sc["name"] for sc in case["acc"]["surfaces"]] and len(kept_cls):
            # one point more than the fold's item in ONE zone, where a sample of the grid finds the zone most often; 2000 others
            n = PZ_ITEM + 1 + 2000
            x, y = rc.uniform(g["min_x"], g["max_x"], n), rc.uniform(g["min_y"], g["max_y"], n)
            cls = kept_cls[rc.integers(0, len(kept_cls), n)]
            if e0["label"] in po["names"]:
                import points_in_polygons_common as PIP
                j = po["names"].index(e0["label"])
                st = po["sets"][j][cur_of[k][j]]
                zs = zones_of(PIP.model(st["polys"], x[:4000], y[:4000], np.float32(st["opts"]["background"])))
                zs[zs > e0["max_zones"]] = 0
                if zs.any():
                    at = np.flatnonzero(zs == np.bincount(zs[zs > 0]).argmax())
                    pick = at[rc.integers(0, len(at), PZ_ITEM + 1)]
                    x[2000:], y[2000:] = x[pick], y[pick]
            elif e0["label"] == "cls":
                zone = kept_cls[kept_cls >= 1]
                cls[2000:] = zone[0] if len(zone) else cls[2000:]
            c = clouds[k] = dict(shape=kind, x=x, y=y, cls=cls, a=(rc.integers(-16, 17, n) / 8.0).astype(np.float32),
                                 b=rc.integers(0, 16, n).astype(np.float32), t=rc.integers(0, 6, n).astype(np.float32))
            _draw_z(rc, g, c, field, case["acc"]["shift"])
        elif kind == "pipeline_emptied":
            n = len(c["x"])
            dropped = cls4[~keep_mask(filt, cls4)]
            c["shape"] = kind
            if len(dropped):
                c["cls"] = dropped[rc.integers(0, len(dropped), n)]
            elif po["clip"]:                                     # far from every polygon: the background, which most clips drop
                c["x"] = rc.uniform(g["max_x"] + 1000 * cs, g["max_x"] + 2000 * cs, n)
        n = len(c["x"])
        if lab_entries:                                          # whole numbers up to max_zones, every invalid label; in one cloud of three a few above
            import point_zonal_common as PZC
            Z = lab_entries[0]["max_zones"]
            lab = rc.integers(1, min(Z, 64) + 1, n).astype(np.float32)
            wide = rc.uniform(size=n) < 0.2
            lab[wide] = rc.integers(1, Z + 1, int(wide.sum()))
            bad = rc.uniform(size=n) < 0.1
            lab[bad] = np.array(PZC.INVALID, np.float32)[rc.integers(0, len(PZC.INVALID), int(bad.sum()))]
            if n and rc.uniform() < 1 / 3:
                lab[rc.integers(0, n, 1 + n // 500)] = Z + rc.integers(1, 4)
            if kind == "hot_zone" and e0["label"] == "lab":
                lab[2000:] = min(Z, 2)
            c["lab"] = lab
        # a share outside the grid and inside a polygon: into the outer part of a half-outside rectangle of channel 0
        rects = [st["opts"]["rect"] for st in po["sets"][0]]
        rect = rects[cur_of[k][0]] if k in cur_of else rects[0]
        share = 0.005 if c["shape"] in ("hot", "hot_acc", "hot_zone") else 0.04
        move = np.flatnonzero(rc.uniform(size=n) < share)
        if len(move) and kind != "pipeline_emptied":
            rx0, ry0, rx1, ry1 = rect
            if rx1 > g["max_x"]:
                c["x"][move], c["y"][move] = rc.uniform(g["max_x"] + 0.01 * cs, rx1, len(move)), rc.uniform(ry0, ry1, len(move))
            else:
                c["x"][move], c["y"][move] = rc.uniform(rx0, rx1, len(move)), rc.uniform(g["max_y"] + 0.01 * cs, ry1, len(move))
    # the exactness condition again, on the clouds as they are now (a replaced cloud is new to the sums)
    units = np.zeros((2, W * H))
    for c in clouds:
        while (units + point_units(g, [c])).max() >= EXACT_UNITS:
            _thin(c, np.arange(len(c["x"])) % 2 == 0)
        units += point_units(g, [c])


POLY_SITUATIONS = ("a polygon channel as a point zonal label, with counted points outside the grid",
                   "set_polygons behind an unsynchronised async ingest", "set_polygons before a larger cloud than any so far",
                   "a polygon channel in the pipeline filter", "a polygon channel in a reduction's filter",
                   "a polygon channel in a point zonal spec's filter", "a polygon channel as a histogram's value channel",
                   "ingest_file in more than one chunk with a polygon-labelled entry",
                   "a cloud the pipeline filter empties between two point_tables",
                   "a spec filter that empties a cloud the pipeline filter keeps", "a point zonal overflow and a read after it",
                   "point_tables before the first ingest", "a surface channel as the label", "more than 2^16 kept points in one zone",
                   "set_zones_poly replacing a grid", "a grid replacing set_zones_poly", "polygonize with a Device result",
                   "polygonize refused after an ingest, and valid again after the next finalize",
                   "polygonize valid behind an emptied cloud", "the reburn chain with at least 20 crowns")


def poly_situations(case):
    """The POLY_SITUATIONS that occur in a polygon case, from the case alone: the channels by the models, the crowns of the
    reburn chain by the model of the sequence (only where a reburn is valid at all)."""
    found = set()
    po, ops, plan, acc, specs, g = case["poly"], case["ops"], case["plan"], case["acc"], case["specs"], case["grid"]
    names, pz = po["names"], po["pz"]
    uses = lambda f: any(p["ch"] in names for p in f or ())
    if any(uses(s["filt"]) for s in specs):
        found.add("a polygon channel in a reduction's filter")
    if any(uses(s["filt"]) for e in pz for s in e["stats"] + e["hists"]):
        found.add("a polygon channel in a point zonal spec's filter")
    if any(h["ch"] in names for h in acc["hist"] + [h for e in pz for h in e["hists"]]):
        found.add("a polygon channel as a histogram's value channel")
    if any(e["label"] in [sc["name"] for sc in acc["surfaces"]] for e in pz):
        found.add("a surface channel as the label")
    cur_at = {i: (k, cur) for i, k, cur in poly_walk(case)}
    finalized = fresh = False
    counted = biggest = 0
    since, pending, zone_kind = set(), False, {}
    over = [False] * len(pz)
    tables_seen = emptied_since_tables = False
    refused_after_ingest = False
    valid_reburn = False
    for i, o in enumerate(ops):
        prev = ops[i - 1] if i else None
        if o["op"] == "ingest":
            k, cur = cur_at[i]
            c = case["clouds"][k]
            n = len(c["x"])
            if n == 0:
                continue
            if pending and biggest and n > biggest:
                found.add("set_polygons before a larger cloud than any so far")
            pending, biggest = False, max(biggest, n)
            ch = cloud_channels(case, k, cur)
            keep = pipeline_keep(case, ch)
            if not keep.any():
                since.add("emptied")
                emptied_since_tables = emptied_since_tables or (tables_seen and counted > 0)
                continue
            if po["clip"] and keep.sum() < keep_mask(case["filt"], c["cls"]).sum():
                found.add("a polygon channel in the pipeline filter")
            counted, fresh, since = counted + 1, False, set()
            tables_seen = emptied_since_tables = False
            outside = cells_of(g, c["x"], c["y"]) < 0
            chunk = max(1, int(n * o["chunk_frac"])) if o["how"] == "file" else n
            for j, e in enumerate(pz):
                zs = zones_of(ch[e["label"]])
                if e["label"] in names and (keep & outside & (zs > 0)).any():
                    found.add("a polygon channel as a point zonal label, with counted points outside the grid")
                if e["label"] in names and chunk < n:
                    found.add("ingest_file in more than one chunk with a polygon-labelled entry")
                if any(s["filt"] and not (keep & conj_mask(ch, s["filt"], n)).any() for s in e["stats"] + e["hists"]):
                    found.add("a spec filter that empties a cloud the pipeline filter keeps")
                if (keep & (zs > e["max_zones"])).any():
                    over[j] = True
                inz = zs[keep & (zs > 0) & (zs <= e["max_zones"])]
                if len(inz) and np.bincount(inz).max() > PZ_ITEM:
                    found.add("more than 2^16 kept points in one zone")
        elif o["op"] == "finalize":
            finalized = fresh = True
            since = set()
            if refused_after_ingest:
                found.add("polygonize refused after an ingest, and valid again after the next finalize")
        elif o["op"] == "set_polygons":
            pending = True
            if prev is not None and prev["op"] == "ingest" and prev["how"].startswith("async") and not prev["sync"] and len(case["clouds"][prev["cloud"]]["x"]):
                found.add("set_polygons behind an unsynchronised async ingest")
        elif o["op"] == "point_tables":
            if not any(q["op"] == "ingest" for q in ops[:i]):
                found.add("point_tables before the first ingest")
            if emptied_since_tables:
                found.add("a cloud the pipeline filter empties between two point_tables")
            tables_seen, emptied_since_tables = True, False
        elif o["op"] == "set_zones":
            zname = [q for q in plan["zonal"] if q["external"]][o["entry"]]["zones"]
            if zone_kind.get(zname) == "poly":
                found.add("a grid replacing set_zones_poly")
            zone_kind[zname] = "grid"
        elif o["op"] == "set_zones_poly":
            zname = plan["zonal"][o["zonal"]]["zones"]
            if zone_kind.get(zname) == "grid":
                found.add("set_zones_poly replacing a grid")
            zone_kind[zname] = "poly"
        elif o["op"] in ("polygonize", "reburn"):
            real = o["band"] != "nope"
            if real and finalized and fresh:
                if plan["loc"] == "Device":
                    found.add("polygonize with a Device result")
                if "emptied" in since:
                    found.add("polygonize valid behind an emptied cloud")
                valid_reburn = valid_reburn or o["op"] == "reburn"
            elif real and finalized:
                refused_after_ingest = True
    if any(over):                                                # (the runner reads every table behind every finalize: the last op is one)
        found.add("a point zonal overflow and a read after it")
    if valid_reburn and reburn_crowns(case) >= 20:
        found.add("the reburn chain with at least 20 crowns")
    return found


def reburn_crowns(case):
    """The most crowns a valid reburn of the case burns: the rows of the tree table of the model's last finalize then."""
    model, most = Model(case), 0
    for o in case["ops"]:
        if o["op"] == "ingest":
            model.ingest(case["clouds"][o["cloud"]])
        elif o["op"] == "set_polygons":
            model.current[o["channel"]] = 1
        elif o["op"] == "planes_write":
            model.patch(o)
        elif o["op"] == "finalize":
            model.leaving_bands(case["plan"])
        elif o["op"] == "reburn" and model.finalized is not None and model.fresh:
            most = max(most, len(model.finalized[2][int(o["band"][1:].split("_")[0])]["row"]))
    return most


# The polygon cases of the suite: a greedy cover of 20000..20999 in which every entry above occurs three times, cheaper cases first
# (tests/test_sequence_fuzz_host.py counts).  A failing seed of a soak joins it.
POLY_SEEDS = [
    20026,  # 2^16 + 1 kept points in one zone; the reburn chain with 20 crowns and more; polygonize with a Device result
    20264,  # ingest_file in chunks with a polygon-labelled entry; a polygon channel in the pipeline filter; a Device result
    20359,  # chunks with a polygon-labelled entry; polygonize refused after an ingest; a grid and a polygon set replacing each other
    20428,  # chunks with a polygon-labelled entry; set_polygons before the largest cloud so far; a polygon predicate in a spec's filter
    20459,  # the reburn chain; a point zonal overflow and reads after it; a spec filter that empties a cloud
    20578,  # 2^16 + 1 kept points in one zone; point_tables before the first ingest; a polygon channel in the pipeline filter
    20671,  # polygonize refused after an ingest and valid after the next finalize; a grid and a polygon set replacing each other
    20690,  # a surface channel as the label; set_polygons before the largest cloud so far; polygonize with a Device result
    20730,  # 2^16 + 1 kept points in one zone; polygonize refused after an ingest; set_zones_poly replacing a grid
    20773,  # a grid replacing set_zones_poly; set_polygons before the largest cloud so far; polygonize with a Device result
    20794,  # polygonize valid behind an emptied cloud; an emptied cloud between two point_tables; set_polygons behind an unwaited ingest_async
    20820,  # an emptied cloud between two point_tables; set_polygons behind an unwaited ingest_async; an overflow
    20876,  # the reburn chain; point_tables before the first ingest; a polygon predicate in a spec's filter
    20890,  # set_polygons behind an unwaited ingest_async; a polygon channel in the pipeline filter and in a reduction's
    20908,  # an emptied cloud between two point_tables; a surface channel as the label; polygonize valid behind an emptied cloud
    20925,  # a surface channel as the label; polygonize valid behind an emptied cloud; set_zones_poly replacing a grid
]


# ---- the model -------------------------------------------------------------------------------------------------------------------
class Model:
    """Per group four float32 planes (sum, count, max, min) or the MostRecent word plane of most_recent_common; one touched-tile
    set; the count of the filter's survivors since the pipeline was created."""
    IDENTITY = (np.float32(0.0), np.float32(0.0), -FLT_MAX, FLT_MAX)

    def __init__(self, case):
        g = case["grid"]
        self.case, self.g, self.W, self.H = case, g, g["W"], g["H"]
        self.tx, self.ty = -(-g["W"] // g["tw"]), -(-g["H"] // g["th"])
        self.touched = np.zeros((self.ty, self.tx), bool)
        self.survivors = 0
        self.og = oracle_grid(g) if case["line"] else None
        self.acc = case.get("acc")
        if self.acc:                                             # the accumulator states, integer arrays as the accessors hand them out
            import extremes_common as E
            a = self.acc
            self.cubes = [np.zeros((h["bins"], self.H, self.W), np.uint32) for h in a["hist"]]
            self.keys = [np.full((e["k"], self.H, self.W), E.EMPTY, np.uint32) for e in a["ext"]]
            self.stats = [(np.zeros((self.H, self.W), np.uint32), np.zeros((self.H, self.W), np.int64), np.zeros((self.H, self.W), np.uint64))
                          for _ in a["stats"]]
            self.version = 0                                     # counts the ingests that changed an accumulator's input
            self.fresh = False                                   # zonal tables: a finalize with no ingest since
            self.finalized = None                                # (names, bands, tree tables) of the last finalize
            self.zones = {}                                      # external label grids that were set
            self._cache = {}
        self.poly = case.get("poly")
        if self.poly:                                            # the current set per channel; per point zonal entry the points of every
            self.current = [0] * len(self.poly["names"])         # ingest that counted: (label, kept, [(mask, value) per spec])
            self.pz = [[] for _ in self.poly["pz"]]
            self.cloud_index = {id(c): k for k, c in enumerate(case["clouds"])}
            self.finalizes = 0
            self.burnt = {}                                      # twin entry -> the finalize its zones were burnt from
        self.planes = []
        for gr in case["groups"]:
            if gr["select"]:
                self.planes.append(np.zeros(self.W * self.H, np.uint64))
            else:
                self.planes.append([np.full(self.W * self.H, self.IDENTITY[p], np.float32) for p in range(4)])

    def touched_cells(self):
        g = self.g
        return np.repeat(np.repeat(self.touched, g["th"], 0), g["tw"], 1)[:self.H, :self.W].reshape(-1)

    def ingest(self, c):
        import most_recent_common as MR
        import pcr_oracle_py as O
        keep = keep_mask(self.case["filt"], c["cls"])
        ch = None
        if self.poly:                                            # the derived channels first: PipelineConfig::filter may name one
            ch = cloud_channels(self.case, self.cloud_index[id(c)], tuple(self.current))
            keep = pipeline_keep(self.case, ch)
        self.survivors += int(keep.sum())
        cell = cells_of(self.g, c["x"], c["y"])
        ok = keep & (cell >= 0)
        cell_ok = cell[ok]
        rows, cols = cell_ok // self.W, cell_ok % self.W
        # (section 18's flag rule: the pipeline filter's survivors alone set the touched flags)
        self.touched[rows // self.g["th"], cols // self.g["tw"]] = True
        if self.acc:
            if keep.any():                                       # (a cloud the pipeline filter empties changes nothing: pipeline.h, Pipeline::zonal)
                self._ingest_acc(c, keep, ch)
            return
        for gr, pl in zip(self.case["groups"], self.planes):
            v = c[gr["ch"]]
            if gr["select"]:
                MR.fold_words(cell, v, c["t"], self.W * self.H, keep=keep, words=pl)
                continue
            if gr["glyph"] is not None:
                # a Line group: the oracle's Sum and Count bands of the kept points through the group's glyph (a NaN: nothing
                # here) added to planes 0 and 1 -- in binary64, exact by the condition of _line_pass.  Nothing else: the
                # footprint is clipped to the centre cell's reference tile (Q4), whose flag is set above
                for p, rtype in ((0, O.SUM), (1, O.COUNT)):
                    if p in gr["slots"] and ok.any():
                        band = np.nan_to_num(oracle_line(self.og, gr["glyph"], rtype, c, v, ok)).reshape(-1)
                        pl[p][:] = (pl[p].astype(np.float64) + band.astype(np.float64)).astype(np.float32)
                continue
            # (binary64 holds every partial sum exactly, and the total is a binary32 number: the condition of build())
            pl[0][:] = (pl[0].astype(np.float64) + np.bincount(cell_ok, v[ok].astype(np.float64), self.W * self.H)).astype(np.float32)
            pl[1][:] = (pl[1].astype(np.float64) + np.bincount(cell_ok, minlength=self.W * self.H)).astype(np.float32)
            np.maximum.at(pl[2], cell_ok, v[ok])
            np.minimum.at(pl[3], cell_ok, v[ok])

    def _ingest_acc(self, c, keep, ch=None):
        """An accumulator case's ingest: the surface channels first, then every group under its own filter AND the pipeline's
        (Max and Min skip a NaN value: fmaxf / fminf), then the accumulators by their *_common models from the same routing."""
        import cell_stats_common as CS
        import extremes_common as E
        import histogram_common as HC
        import most_recent_common as MR
        a, g, n = self.acc, self.g, len(c["x"])
        self.version += 1
        self.fresh = False
        ch = surface_channels(a, c) if ch is None else ch
        cell = cells_of(g, c["x"], c["y"])
        # a polygon case's point zonal entries: label, PipelineConfig::filter's mask and per spec its mask and value, of ALL n
        # points -- the grid plays no part
        for e, chunks in zip(self.poly["pz"] if self.poly else (), self.pz if self.poly else ()):
            chunks.append((ch[e["label"]], keep, [(keep & conj_mask(ch, sp["filt"], n), ch[sp["ch"]]) for sp in e["stats"] + e["hists"]]))
        for gr, pl in zip(self.case["groups"], self.planes):
            mine = keep & conj_mask(ch, gr["filt"], n)
            v = ch[gr["ch"]]
            if gr["select"]:
                MR.fold_words(cell, v, c["t"], self.W * self.H, keep=mine, words=pl)
                continue
            ok = mine & (cell >= 0)
            pl[0][:] = (pl[0].astype(np.float64) + np.bincount(cell[ok], v[ok].astype(np.float64), self.W * self.H)).astype(np.float32) \
                if gr["ch"] in ("a", "b") else pl[0]
            pl[1][:] = (pl[1].astype(np.float64) + np.bincount(cell[ok], minlength=self.W * self.H)).astype(np.float32)
            np.fmax.at(pl[2], cell[ok], v[ok])
            np.fmin.at(pl[3], cell[ok], v[ok])
        for i, h in enumerate(a["hist"]):
            with np.errstate(over="ignore"):
                self.cubes[i] += HC.cube(g, c["x"], c["y"], ch[h["ch"]], h["lo"], h["hi"], h["bins"], keep & conj_mask(ch, h["filt"], n))
        for i, e in enumerate(a["ext"]):
            new = E.planes(g, c["x"], c["y"], ch[e["ch"]], e["k"], e["side"], keep & conj_mask(ch, e["filt"], n))
            both = np.sort(np.concatenate([self.keys[i], new]), axis=0)       # the k smallest DISTINCT keys of the union
            both[1:][both[1:] == both[:-1]] = E.EMPTY
            self.keys[i] = np.sort(both, axis=0)[:e["k"]]
        for i, s in enumerate(a["stats"]):
            self.stats[i] = CS.planes(g, c["x"], c["y"], ch[s["ch"]], s["origin"], s["res"], keep & conj_mask(ch, s["filt"], n), into=self.stats[i])

    def acc_raw_bands(self):
        """The accumulator bands as finalize makes them, in acc_bands' order (cached per state: the cell-stats model walks every
        non-empty cell with Python ints)."""
        import cell_stats_common as CS
        import extremes_common as E
        import histogram_common as HC
        if self._cache.get("bands_version") != self.version:
            a, out = self.acc, []
            for h, cube in zip(a["hist"], self.cubes):
                out += HC.percentiles(cube, h["lo"], h["hi"], h["bins"], h["qs"])
            out += [E.band(keys, e["side"], e["gap"]) for e, keys in zip(a["ext"], self.keys)]
            for s, st in zip(a["stats"], self.stats):
                made = CS.bands(*st, s["origin"], s["res"], s["ddof"])
                out += [made[p] for p in s["products"]]
            self._cache["bands_version"], self._cache["bands"] = self.version, out
        return [b.copy() for b in self._cache["bands"]]

    def patch(self, o):
        r0, c0, h, w = o["rect"]
        pl = self.planes[o["group"]][o["slot"]].reshape(self.H, self.W)
        pl[r0:r0 + h, c0:c0 + w] += np.float32(o["value"])

    def flag(self, tiles):
        for r, c in tiles:
            self.touched[r, c] = True

    def snapshot(self):
        """What save_state writes: the planes of the touched tiles."""
        return [pl.copy() if gr["select"] else [q.copy() for q in pl] for gr, pl in zip(self.case["groups"], self.planes)], self.touched.copy()

    def overlay(self, snap):
        """load_state: the tiles of the checkpoint replace the state's, their flags are set; every other tile stays."""
        planes, touched = snap
        g = self.g
        cells = np.repeat(np.repeat(touched, g["th"], 0), g["tw"], 1)[:self.H, :self.W].reshape(-1)
        for gr, pl, src in zip(self.case["groups"], self.planes, planes):
            if gr["select"]:
                pl[cells] = src[cells]
            else:
                for p in range(4):
                    pl[p][cells] = src[p][cells]
        self.touched |= touched

    def carried_over(self):
        """What a checkpoint carries into a new pipeline: the touched tiles.  A cell of an untouched tile is the identity again."""
        gone = ~self.touched_cells()
        for gr, pl in zip(self.case["groups"], self.planes):
            if gr["select"]:
                pl[gone] = 0
            else:
                for p in range(4):
                    pl[p][gone] = self.IDENTITY[p]
        self.survivors = 0

    def state_planes(self):
        """{(group, slot): the plane as state_planes() and the checkpoints show it}"""
        import most_recent_common as MR
        out = {}
        for gi, (gr, pl) in enumerate(zip(self.case["groups"], self.planes)):
            if gr["select"]:
                out[(gi, 0)], out[(gi, 1)] = MR.state_of_words(pl, (self.H, self.W))
            else:
                for p in sorted(gr["slots"]):
                    out[(gi, p)] = pl[p].reshape(self.H, self.W)
        return out

    def raw_bands(self):
        """finalize_rt: Sum as is; Count and Average NaN where the count is 0; Max and Min NaN at the identity; Average one
        binary32 division; every cell of an unflagged tile NaN."""
        import most_recent_common as MR
        live = self.touched_cells()
        out = []
        for s in self.case["specs"]:
            pl = self.planes[s["group"]]
            if s["type"] == "MostRecent":
                band = MR.band_of_words(pl, (self.W * self.H,))
            else:
                sm, ct, mx, mn = pl
                with np.errstate(all="ignore"):
                    band = {"Sum": lambda: sm.copy(), "Count": lambda: np.where(ct > 0, ct, np.float32(np.nan)),
                            "Average": lambda: np.where(ct > 0, sm / ct, np.float32(np.nan)),
                            "WeightedAverage": lambda: np.where(ct > 0, sm / ct, np.float32(np.nan)),      # (weight 1 a visit)
                            "Max": lambda: np.where(mx == -FLT_MAX, np.float32(np.nan), mx),
                            "Min": lambda: np.where(mn == FLT_MAX, np.float32(np.nan), mn)}[s["type"]]()
            band = np.where(live, band, np.float32(np.nan)).astype(np.float32)
            out.append(band.reshape(self.H, self.W))
        return out

    def leaving_bands(self, plan):
        """finalize()'s documented order: the filter on the RAW source band; the fill of the Average / Max / Min / MostRecent
        bands and of the DTM; hag from the bands as they leave.  -> (names, bands)"""
        import ground_filter_common as G
        import pcr
        raw = self.raw_bands()
        names = [band_name(i, s) for i, s in enumerate(self.case["specs"])]
        fills = [i for i, s in enumerate(self.case["specs"]) if s["type"] in FILL_TYPES]
        if self.acc:
            # the documented order: reductions, percentiles, extremes, cell stats -- then dtm, hag, terrain, tree bands; percentile,
            # extremes and Mean bands are filled, Variance and StdDev bands never
            for k, (name, kind, _, _) in enumerate(acc_bands(self.acc)):
                fills += [len(names)] if acc_filled(kind) else []
                names.append(name)
            raw = raw + self.acc_raw_bands()
        out = list(raw)
        if plan["fill"] > 0 and fills:
            filled = G.grid_bands(pcr.fill_nodata(G.make_grid(raw), plan["fill"], fills))
            out = [filled[i] if i in fills else raw[i] for i in range(len(raw))]
        if plan["ground"]:
            spec = pcr.GroundFilterSpec()
            spec.max_radius_cells = plan["ground"]["maxr"]
            source, top = ground_names(self.case["specs"], plan)
            dtm = G.grid_bands(pcr.ground_filter(G.make_grid([raw[names.index(source)]]), 0, spec, self.g["cs"]))[0]
            if plan["fill"] > 0:
                dtm = G.grid_bands(pcr.fill_nodata(G.make_grid([dtm]), plan["fill"]))[0]
            out.append(dtm)
            names.append("dtm")
            if top is not None:
                out.append(G.difference(out[names.index(top)], dtm))
                names.append("hag")
        # the terrain bands, in list order behind dtm / hag: each from its source band as it leaves (filled), by the NumPy
        # restatement of the contract (no engine code but the light constants, which are the contract), never filled themselves
        if plan.get("terrain"):
            import terrain_common as T
            leaving = dict(zip(names, out))
            for t in plan["terrain"]:
                out.append(T.terrain(leaving[t["source"]], [T.PRODUCTS[TERRAIN_PRODUCTS.index(t["product"])]], z_factor=t["z_factor"],
                                     edges=t["edges"], azimuth=t["azimuth"], altitude=t["altitude"], cell_size_x=self.g["cs"],
                                     cell_size_y=-self.g["cs"])[0])
                names.append(terrain_band_name(t))
        # the tree bands, two per entry behind the terrain bands: from the source as it leaves, by the host twin (which
        # tests/test_trees.py holds to the brute-force model); the table's centres by the grid's geometry
        tables = []
        for i, t in enumerate(plan.get("trees") or []):
            import trees_common as TR
            got = TR.host(out[names.index(t["source"])], TR.spec(**TREE_KW[t["kw"]]), self.g["cs"], -self.g["cs"])
            tab = got["table"]
            tab["x"] = self.g["min_x"] + (tab["col"].astype(np.float64) + 0.5) * self.g["cs"]
            tab["y"] = self.g["max_y"] + (tab["row"].astype(np.float64) + 0.5) * -self.g["cs"]
            out += [got["id"], got["height"]]
            names += [f"t{i}_id", f"t{i}_h"]
            tables.append(tab)
        if self.acc:
            self.fresh, self.finalized = True, (names, out, tables)
        if self.poly:
            self.finalizes += 1
        return names, out

    def point_zonal_table(self, i):
        """Pipeline::point_zonal of entry i: (table, [counts per histogram]) by point_zonal_common.table_masked on the points of
        every ingest that counted, concatenated (the bits depend on the multiset of points only) -- or the OutOfRange message
        once a kept point carried a zone above max_zones, whatever its value.  Points that PipelineConfig::filter drops or
        that carry no zone add nothing to any word: they are left out of the Python-int walk."""
        import point_zonal_common as PZC
        e, chunks = self.poly["pz"][i], self.pz[i]
        if self._cache.get(("pz", i), (None,))[0] != len(chunks):
            specs = e["stats"] + e["hists"]
            cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
            labels, base = cat([c[0] for c in chunks], np.float32), cat([c[1] for c in chunks], bool)
            zs = zones_of(labels)
            over = int((base & (zs > e["max_zones"])).sum())
            if over:
                ans = f"{over} points of '{e['label']}' carry a zone above max_zones = {e['max_zones']}"
            else:
                sel = base & (zs > 0)
                cols = [(cat([c[2][k][0] for c in chunks], bool)[sel], cat([c[2][k][1] for c in chunks], np.float32)[sel]) for k in range(len(specs))]
                stats = [(sp["ch"], v, m, sp["origin"], sp["res"], sp["ddof"]) for sp, (m, v) in zip(e["stats"], cols)]
                hists = [(sp["ch"], v, m, sp["lo"], sp["hi"], sp["bins"], sp["qs"]) for sp, (m, v) in zip(e["hists"], cols[len(e["stats"]):])]
                ans = PZC.table_masked(labels[sel], e["max_zones"], None, stats=stats, hists=hists)
            self._cache[("pz", i)] = (len(chunks), ans)
        return self._cache[("pz", i)][1]

    def outline(self, name):
        """Pipeline::polygonize: the polygon set of polygonize_common.model on the band as the last finalize left it, under
        zonal's condition (a finalize with no ingest since) -- or the message of the documented refusal."""
        import polygonize_common as PG
        if self.finalized is None or not self.fresh:
            return f"no band '{name}' \\(of a finalize with no ingest since\\)"
        if name not in self.finalized[0]:
            return f"'{name}' names no Float32 band of the result"
        band = self.finalized[1][self.finalized[0].index(name)]
        key = ("outline", bits_key(band))
        if key not in self._cache:
            self._cache[key] = PG.set_of(PG.model(band), grid_geom(self.g))
        return self._cache[key]

    def burn(self, polys, background):
        """set_zones(name, polygons): rasterize_common.model on the pipeline's grid."""
        import rasterize_common as RC
        return RC.model(polys, grid_geom(self.g), background)

    def acc_states(self):
        """What histogram(i), extremes(i) and cell_stats(i) answer: the cubes, the decoded key planes, (N, S1, S2)."""
        import extremes_common as E
        return (self.cubes, [E.value_of(k, e["side"]) for k, e in zip(self.keys, self.acc["ext"])], self.stats)

    def trees_table(self, i):
        """Pipeline::trees: the table of the last finalize, whatever came since; before the first: the refusal."""
        return "no trees entry" if self.finalized is None else self.finalized[2][i]

    def zonal_table(self, plan, i):
        """Pipeline::zonal of entry i: (table, [counts per chosen histogram]) by zonal_common's Python-int model on the labelled
        cells' bounding box (a cell without a zone adds nothing to any row), or the message of the documented refusal."""
        import zonal_common as Z
        z, a = plan["zonal"][i], self.acc
        if self.finalized is None or not self.fresh:
            return f"no zonal entry {i} \\(of a finalize with no ingest since\\)"
        if z["external"]:
            if z["zones"] not in self.zones:
                return f"the label grid '{z['zones']}' was not set"
            labels = self.zones[z["zones"]]
        else:
            labels = self.finalized[1][self.finalized[0].index(z["zones"])]
        key = (self.version, bits_key(labels))                   # (the states and the labels: all the table is made of)
        if self._cache.get("zonal_key", {}).get(i) != key:
            with np.errstate(all="ignore"):
                valid = np.isfinite(labels) & (labels >= 1) & (labels <= Z.MAX_ZONE) & (labels == np.floor(labels))
            if valid.any():
                rr, cc = np.nonzero(valid)
                box = (slice(rr.min(), rr.max() + 1), slice(cc.min(), cc.max() + 1))
            else:
                box = (slice(0, 1), slice(0, 1))
            zmax = Z.zone_max(labels[box])
            if zmax > z["max_zones"]:
                ans = f"is above max_zones = {z['max_zones']}"
            else:
                stats = [(a["stats"][k]["ch"], tuple(p[box] for p in self.stats[k]), a["stats"][k]["origin"], a["stats"][k]["res"], a["stats"][k]["ddof"])
                         for k in z["stats"]]
                hists = [(a["hist"][k]["ch"], self.cubes[k][(slice(None),) + box], *Z.hist_consts(a["hist"][k]["lo"], a["hist"][k]["hi"], a["hist"][k]["bins"]),
                          a["hist"][k]["qs"] if z["own"] else z["qs"]) for k in z["hists"]]
                ans = Z.table(labels[box], stats=stats, hists=hists)
            self._cache.setdefault("zonal_key", {})[i] = key
            self._cache.setdefault("zonal", {})[i] = ans
        return self._cache["zonal"][i]

    def write_checkpoint(self, dirname):
        """The model's state as `.pcrt` files in the pipelines' layout: one file per touched tile and reduction."""
        import pcr
        planes = self.state_planes()
        specs, g = self.case["specs"], self.g
        for r, s in enumerate(specs):
            rdir = dirname if len(specs) == 1 else os.path.join(dirname, f"reduction_{r}")
            os.makedirs(rdir, exist_ok=True)
            for tr, tc in np.argwhere(self.touched):
                r0, c0 = tr * g["th"], tc * g["tw"]
                state = np.stack([planes[(s["group"], p)][r0:r0 + g["th"], c0:c0 + g["tw"]] for p in PLANES_OF[s["type"]]])
                pcr.write_tile_state(pcr.tile_state_filename(rdir, int(tr), int(tc)), int(tr), int(tc),
                                     np.ascontiguousarray(state, np.float32), getattr(pcr.ReductionType, s["type"]))


def band_name(i, s):
    return f"r{i}_{s['type']}_{s['ch']}"


def bits_key(a):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def overview_level_count(W, H):
    n, f = 0, 2
    while min(W, H) // f >= 256:                                 # write_cog's rule (the reference's): levels 2, 4, ... while min(W, H) / level >= 256
        n, f = n + 1, f * 2
    return n


# ---- the runner ------------------------------------------------------------------------------------------------------------------
def bytes_per_row(case):
    """Pipeline::Banded::bytes_per_row: 4 B per cell and plane (a MostRecent group: its two slots), + the finalized bands."""
    return case["grid"]["W"] * 4 * (sum(len(gr["slots"]) for gr in case["groups"]) + len(case["specs"]))


def make_config(case, plan, flavour, exec_mode, engine, tmp_path, state_dir=None):
    import pcr
    g = case["grid"]
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(g["min_x"], g["min_y"], g["max_x"], g["max_y"])
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = g["cs"], -g["cs"]
    cfg.grid.tile_width, cfg.grid.tile_height = g["tw"], g["th"]
    cfg.grid.compute_dimensions()
    assert (cfg.grid.width, cfg.grid.height) == (g["W"], g["H"])
    cfg.exec_mode = exec_mode
    reds = []
    for i, s in enumerate(case["specs"]):
        r = pcr.ReductionSpec()
        r.value_channel, r.type, r.output_band_name = s["ch"], getattr(pcr.ReductionType, s["type"]), band_name(i, s)
        if s["type"] == "MostRecent":
            r.timestamp_channel = "t"
        if "glyph" in s:
            gl = pcr.GlyphSpec()
            gl.type, gl.direction_channel, gl.half_length_channel = pcr.GlyphType.Line, "dir", s["glyph"]["hl_ch"]
            gl.default_half_length, gl.max_radius_cells = s["glyph"]["hl"], s["glyph"]["maxr"]
            r.glyph = gl
        if s.get("filt"):
            r.filter = filter_spec(s["filt"])
        reds.append(r)
    cfg.reductions = reds
    if case.get("poly"):                                         # PipelineConfig::filter: the `cls` predicate, then the clip
        first = [dict(case["filt"], ch="cls")] if case["filt"] else []
        if first or case["poly"]["clip"]:
            cfg.filter = filter_spec(first + case["poly"]["clip"])
        poly_config(pcr, cfg, case["poly"])
    elif case["filt"]:
        f = pcr.FilterSpec()
        if case["filt"]["op"] in ("InSet", "NotInSet"):
            pr = pcr.FilterPredicate()
            pr.channel_name, pr.op, pr.value_set = "cls", getattr(pcr.CompareOp, case["filt"]["op"]), case["filt"]["set"]
            f.predicates = [pr]
        else:
            f.add("cls", getattr(pcr.CompareOp, case["filt"]["op"]), case["filt"]["value"])
        cfg.filter = f
    cfg.fill_nodata_radius = plan["fill"]
    if plan["ground"]:
        cfg.ground.source_band, top = ground_names(case["specs"], plan)
        if top is not None:
            cfg.ground.top_band = top
        cfg.ground.max_radius_cells = plan["ground"]["maxr"]
    if case.get("acc"):
        acc_config(pcr, cfg, case["acc"], plan)
    if plan.get("terrain"):
        import terrain_common as T
        cfg.terrain = [T.band_cfg(t["source"], T.PRODUCTS[TERRAIN_PRODUCTS.index(t["product"])], t["name"], z_factor=t["z_factor"],
                                  compute_edges=t["edges"], azimuth=t["azimuth"], altitude=t["altitude"]) for t in plan["terrain"]]
    ooc = flavour["ooc"] and engine == "hip"
    if plan["loc"] == "Device" and engine == "hip" and not ooc:
        cfg.result_location = pcr.MemoryLocation.Device
    if plan["out"]:
        cfg.output_path, cfg.write_cog = str(tmp_path / "out.tif"), plan["cog"]
    cfg.finalize_with_first_ingest = case["fwfi"]
    cfg.scatter_path = case["path"]
    if ooc:                                                      # a device budget of two or three row bands of whole tile rows
        tile_rows = -(-g["H"] // g["th"])
        cfg.gpu_memory_budget = bytes_per_row(case) * g["th"] * -(-tile_rows // flavour["bands"]) + 64
        cfg.host_cache_budget = flavour["host_budget"]
        cfg.state_dir = str(tmp_path / "work")
    if state_dir is not None:
        cfg.state_dir, cfg.resume = state_dir, True
    return cfg


def filter_spec(f):
    import pcr
    out = pcr.FilterSpec()
    preds = []
    for q in f:
        pr = pcr.FilterPredicate()
        pr.channel_name, pr.op = q["ch"], getattr(pcr.CompareOp, q["op"])
        if q["op"] in ("InSet", "NotInSet"):
            pr.value_set = q["set"]
        else:
            pr.value = q["value"]
        preds.append(pr)
    out.predicates = preds
    return out


def acc_config(pcr, cfg, acc, plan):
    """The lists of an accumulator case, every band named as acc_bands names it."""
    import trees_common as TR
    cfg.surface_channels = [pcr.SurfaceChannelConfig(sc["name"], sc["value"], pcr.SampleMode.Bilinear if sc["mode"] else pcr.SampleMode.Nearest)
                            for sc in acc["surfaces"]]
    names = [n for n, _, _, _ in acc_bands(acc)]
    at, hs, xs, cs = 0, [], [], []
    for h in acc["hist"]:
        e = pcr.HistogramConfig(h["ch"], h["lo"], h["hi"], h["bins"], [float(q) for q in h["qs"]])
        e.band_names = names[at:at + len(h["qs"])]
        at += len(h["qs"])
        if h["filt"]:
            e.filter = filter_spec(h["filt"])
        hs.append(e)
    for x in acc["ext"]:
        e = pcr.ExtremesConfig(x["ch"], pcr.ExtremeSide.Highest if x["side"] else pcr.ExtremeSide.Lowest, x["k"], x["gap"])
        e.band_name = names[at]
        at += 1
        if x["filt"]:
            e.filter = filter_spec(x["filt"])
        xs.append(e)
    kinds = (pcr.CellStat.Mean, pcr.CellStat.Variance, pcr.CellStat.StdDev)
    for c in acc["stats"]:
        e = pcr.CellStatsConfig(c["ch"], origin=c["origin"], resolution=c["res"], products=[kinds[k] for k in c["products"]], ddof=c["ddof"])
        e.band_names = names[at:at + len(c["products"])]
        at += len(c["products"])
        if c["filt"]:
            e.filter = filter_spec(c["filt"])
        cs.append(e)
    cfg.histograms, cfg.extremes, cfg.cell_stats = hs, xs, cs
    cfg.trees = [TR.band_cfg(t["source"], f"t{i}_id", f"t{i}_h", **TREE_KW[t["kw"]]) for i, t in enumerate(plan["trees"])]
    cfg.zonal = [pcr.ZonalConfig(z["zones"], external=z["external"], cell_stats=z["stats"], histograms=z["hists"],
                                 percentiles=None if z["own"] else [float(q) for q in z["qs"]], max_zones=z["max_zones"]) for z in plan["zonal"]]


def poly_config(pcr, cfg, po):
    """The polygon channels and the point zonal entries of a polygon case."""
    cfg.polygon_channels = [pcr.PolygonChannelConfig(n) for n in po["names"]]
    kinds = (pcr.CellStat.Mean, pcr.CellStat.Variance, pcr.CellStat.StdDev)
    entries = []
    for e in po["pz"]:
        st, hs = [], []
        for sp in e["stats"]:
            c = pcr.CellStatsConfig(sp["ch"], origin=sp["origin"], resolution=sp["res"], products=[kinds[2]], ddof=sp["ddof"])
            if sp["filt"]:
                c.filter = filter_spec(sp["filt"])
            st.append(c)
        for sp in e["hists"]:
            h = pcr.HistogramConfig(sp["ch"], sp["lo"], sp["hi"], sp["bins"], [float(q) for q in sp["qs"]])
            if sp["filt"]:
                h.filter = filter_spec(sp["filt"])
            hs.append(h)
        entries.append(pcr.PointZonalConfig(e["label"], st, hs, e["max_zones"]))
    cfg.point_zonal = entries


def set_polygons(p, name, st):
    p.set_polygons(name, st["polys"].to_pcr(), background=st["opts"]["background"], index_cols=st["opts"]["index_cols"],
                   index_rows=st["opts"]["index_rows"])


def _cloud(c, where):
    import pcr
    n = len(c["x"])
    loc = pcr.MemoryLocation.HostPinned if where == "pinned" else pcr.MemoryLocation.Host
    cloud = pcr.PointCloud.create(max(n, 1), loc)
    cloud.set_x_array(np.asarray(c["x"], np.float64))
    cloud.set_y_array(np.asarray(c["y"], np.float64))
    cloud.resize(n)
    for name in cloud_keys(c)[2:]:
        cloud.add_channel(name, pcr.DataType.Float32)
        if n:
            cloud.set_channel_array_f32(name, c[name])
    return cloud.to_device() if where == "device" else cloud


def _same_tree(got_dir, want_dir, what):
    def files(d):
        return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    got, want = files(got_dir), files(want_dir)
    assert got == want, f"{what}: files {sorted(set(got) ^ set(want))[:4]} are in one checkpoint only"
    for f in got:
        assert filecmp.cmp(os.path.join(got_dir, f), os.path.join(want_dir, f), shallow=False), f"{what}: {f} differs from the host engine's file"


def check_sequence(seed, exec_mode, engine, tmp_path):
    """Runs case `seed` on one engine and holds it to the model after every finalize, plane read and checkpoint."""
    import ctypes as C

    import overviews_common as M
    import pcr
    from conftest import load_cabi

    case = build(seed)
    model = Model(case)
    hip = engine == "hip"
    A = load_cabi() if hip else None
    W, H = case["grid"]["W"], case["grid"]["H"]
    plan, flavour = case["plan"], case["flavour"]
    alive = []                                                   # clouds and unions a stream may still read
    snaps = {}                                                   # op index of a checkpoint -> the model's state then

    def create(state_dir=None):
        p = pcr.Pipeline.create(make_config(case, plan, flavour, exec_mode, engine, tmp_path, state_dir))
        assert p is not None, f"seed {seed}: create: {pcr.pipeline_create_error()}"
        assert p.engine() == engine, f"seed {seed}: engine {p.engine()}"
        assert p.out_of_core() == (hip and flavour["ooc"]), f"seed {seed}: out_of_core() is {p.out_of_core()}"
        for sc in (case["acc"] or {}).get("surfaces", ()):       # every surface before the first ingest
            import sample_grid_common as SG
            p.set_surface(sc["name"], SG.pcr_grid(pcr, surface_of(sc)))
        for name, sets in zip(*((case["poly"]["names"], case["poly"]["sets"]) if case["poly"] else ((), ()))):
            set_polygons(p, name, sets[0])                       # every channel's first set before the first ingest, as create requires
        return p

    def refusal(call, message, what):
        try:
            call()
        except RuntimeError as e:
            import re
            assert re.search(message, str(e)), f"{what}: refused with '{e}', not with '{message}'"
            return
        raise AssertionError(f"{what}: answered, the model expects the refusal '{message}'")

    def check_acc(at):
        """histogram(i), extremes(i), cell_stats(i) against the model's states, bit for bit."""
        import cell_stats_common as CS
        import extremes_common as E
        import histogram_common as HC
        cubes, values, stats = model.acc_states()
        for i, want in enumerate(cubes):
            HC.cubes_equal(p.histogram(i), want, f"{at}: histogram({i})")
        for i, want in enumerate(values):
            HC.bits_equal(p.extremes(i), want, f"{at}: extremes({i})")
        for i, want in enumerate(stats):
            CS.planes_equal(p.cell_stats(i), want, f"{at}: cell_stats({i})")

    def check_tables(at):
        """trees(i), zonal(i) and zonal_histogram(i, h) against the model: a table, or the documented refusal."""
        import trees_common as TR
        import zonal_common as Z
        for i in range(len(plan["trees"])):
            want = model.trees_table(i)
            if isinstance(want, str):
                refusal(lambda: p.trees(i), want, f"{at}: trees({i})")
                continue
            got = {k: np.asarray(v) for k, v in p.trees(i).items()}
            for k in TR.COLUMNS:
                a, b = got[k], np.asarray(want[k])
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{at}: trees({i}).{k} differs"
        for i, z in enumerate(plan["zonal"]):
            want = model.zonal_table(plan, i)
            if isinstance(want, str):
                refusal(lambda: p.zonal(i), want, f"{at}: zonal({i})")
                refusal(lambda: p.zonal_histogram(i, 0), want, f"{at}: zonal_histogram({i}, 0)")
                continue
            Z.same_table(p.zonal(i), want[0], f"{at}: zonal({i})")
            for h, counts in enumerate(want[1]):
                Z.bits_equal(p.zonal_histogram(i, h), counts, f"{at}: zonal_histogram({i}, {h})")
            refusal(lambda: p.zonal_histogram(i, len(want[1])), f"no histogram {len(want[1])} in the entry", f"{at}: zonal_histogram({i}, {len(want[1])})")

    def check_point_tables(at, counts=True):
        """point_zonal(i) and point_zonal_histogram(i, h) of every entry against the model: a table, or the OutOfRange message."""
        import point_zonal_common as PZC
        import zonal_common as Z
        for i, e in enumerate(case["poly"]["pz"]):
            want = model.point_zonal_table(i)
            if isinstance(want, str):
                refusal(lambda: p.point_zonal(i), want, f"{at}: point_zonal({i})")
                if counts and e["hists"]:
                    refusal(lambda: p.point_zonal_histogram(i, 0), want, f"{at}: point_zonal_histogram({i}, 0)")
                continue
            Z.same_table(p.point_zonal(i), want[0], f"{at}: point_zonal({i})")
            for h, cnt in enumerate(want[1] if counts else []):
                PZC.bits_equal(p.point_zonal_histogram(i, h), cnt, f"{at}: point_zonal_histogram({i}, {h})")

    def check_outline(at, name):
        import polygonize_common as PG
        want = model.outline(name)
        if isinstance(want, str):
            refusal(lambda: p.polygonize(name), want, f"{at}: polygonize('{name}')")
            return None
        got = p.polygonize(name)
        if want.P == 0:                                          # (no zone in the band: the empty set carries no values)
            assert (got.num_polygons, got.num_rings, got.num_vertices) == (0, 0, 0), f"{at}: polygonize('{name}') of a band without a zone"
            return got
        PG.bits_equal(got, want, f"{at}: polygonize('{name}')")
        return got

    def check_twins(at):
        """The reburn chain: where a twin's zones were burnt from the tree-id band of THIS finalize and both tables answer, the
        twin's table is the by-band entry's, bit for bit -- engine against engine, no model between them."""
        import zonal_common as Z
        for i, z in enumerate(plan["zonal"]):
            if "twin_of" in z and model.burnt.get(i) == model.finalizes and model.fresh and not isinstance(model.zonal_table(plan, i), str):
                got, want = p.zonal(i), p.zonal(z["twin_of"])
                Z.same_table(got, want, f"{at}: zonal({i}), burnt from polygonize('{plan['zonal'][z['twin_of']]['zones']}'), against zonal({z['twin_of']})")
                for h in range(len(z["hists"])):
                    Z.bits_equal(p.zonal_histogram(i, h), p.zonal_histogram(z["twin_of"], h), f"{at}: zonal_histogram({i}, {h}) against the by-band entry's")

    def d2h(ptr, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        A.check(A.lib().pcr_hip_memcpy_d2h(out.ctypes.data, C.c_void_p(ptr), out.nbytes, None))
        A.check(A.lib().pcr_hip_stream_synchronize(None))
        return out

    def h2d(ptr, a):
        a = np.ascontiguousarray(a)
        A.check(A.lib().pcr_hip_memcpy_h2d(C.c_void_p(ptr), a.ctypes.data, a.nbytes, None))
        A.check(A.lib().pcr_hip_stream_synchronize(None))

    p = create()
    first_ingest, expect_deferred = True, False
    for k, o in enumerate(case["ops"]):
        at = f"seed {seed}, op {k} ({o['op']})"
        in_core_hip = hip and not p.out_of_core()
        if o["op"] == "ingest":
            c = case["clouds"][o["cloud"]]
            how = o["how"]
            if how == "file":
                path = str(tmp_path / f"cloud{k}.pcrp")
                pcr.write_point_cloud(path, _cloud(c, "host"))
                chunk = max(1, int(len(c["x"]) * o["chunk_frac"]))
                assert p.ingest_file(path, chunk_points=chunk) == len(c["x"]), f"{at}: points read"
            elif how in ("host", "device"):
                cloud = _cloud(c, how if hip else "host")         # (the host engine: the same cloud from host memory)
                alive.append(cloud)
                p.ingest(cloud)
            else:
                cloud = _cloud(c, ("pinned" if how == "async_pinned" else "device") if hip else "host")
                alive.append(cloud)
                p.ingest_async(cloud)
                if o["sync"]:
                    p.synchronize()
            model.ingest(c)
            if first_ingest and hip and (case["marked"] or case["split_first"]):      # the fuzz reaches the code it is for
                info = p.last_scatter()
                assert info["bands_with_scatter"] > 0, f"{at}: the first ingest stored no bands: {info}"
                if defers_for_sure(case):
                    assert info["deferred_planes"] != 0, f"{at}: the first ingest left no plane in its bands: {info}"
                expect_deferred = defers_for_sure(case) and case["ops"][k + 1] == dict(op="finalize", wait=True)
            first_ingest = False
            # a line case: the Line groups are the last to scatter, so last_scatter() is the last Line group's.  Where the binned
            # path is forced it was taken, and a hot or late-large cloud went through the tile kernels by the engine's own rule
            # too -- in tiles of the side that line_tile_records and line_list_load count with
            special = c["shape"] in ("hot_line", "late_overflow", "late_used") and line_binned(case, o)
            if case["line"] and in_core_hip and (case["path"] == 2 or special) and (keep_mask(case["filt"], c["cls"]) & (cells_of(case["grid"], c["x"], c["y"]) >= 0)).any():
                info = p.last_scatter()
                assert info["path"] == "binned", f"{at}: the Line scatter of a {c['shape']} cloud took the {info['path']} path: {info}"
                last = [gr for gr in case["groups"] if gr["glyph"] is not None][-1]
                side = line_tile(case["grid"], last["glyph"], sum(1 << q for q in last["slots"]))["S"]
                assert info["lds_tile"] == (side, side), f"{at}: Line tiles {info['lds_tile']}, the generator counts with {side}"
        elif o["op"] == "finalize":
            if o["wait"]:
                p.finalize()
            else:
                p.finalize_async()
                p.synchronize()
            if expect_deferred:
                # the blocking finalize right behind the offered ingest has read the done word: 1 (the bands are the scatter's,
                # the planes stay in them) -- or 0 where the scan split a bin: the finalize pass ran, every plane was stored
                left = p.last_scatter()["deferred_planes"]
                assert (left == 0) == case["split_first"], f"{at}: deferred_planes {left} behind a {'split' if case['split_first'] else 'whole'} first ingest"
            expect_deferred = False
            names, want = model.leaving_bands(plan)
            res = p.result()
            assert res is not None, f"{at}: no result"
            host = res if res.location() != pcr.MemoryLocation.Device else res.to_host()
            assert [host.band_desc(b).name for b in range(host.num_bands())] == names, f"{at}: band names"
            for b, name in enumerate(names):
                M.bits_equal(np.array(host.band_array(b)), want[b], f"{at}, band {b} ({name}) of result()")
            for b, name in enumerate(names if in_core_hip else []):
                ptr = p.result_band_device_ptr(b)
                assert ptr != 0, f"{at}: result_band_device_ptr({b})"
                M.bits_equal(d2h(ptr, (H, W)), want[b], f"{at}, band {b} ({name}) of result_band_device_ptr")
            if in_core_hip:
                assert p.result_band_device_ptr(len(names)) == 0, f"{at}: result_band_device_ptr answers one past the last band"
            if plan["out"]:
                tif = str(tmp_path / "out.tif")
                levels = overview_level_count(W, H) if plan["cog"] else 0
                assert pcr.read_geotiff_band_names(tif) == names, f"{at}: GeoTIFF band names"
                assert len(pcr.read_geotiff_overviews(tif)) == levels, f"{at}: GeoTIFF levels"
                for b, name in enumerate(names):
                    M.bits_equal(pcr.read_geotiff_band(tif, b), want[b], f"{at}, band {b} ({name}) of the GeoTIFF")
                    for lv, lw in enumerate(M.pyramid(want[b], levels)):
                        M.bits_equal(pcr.read_geotiff_band(tif, b, lv + 1), lw, f"{at}, band {b} ({name}), level {lv + 1} of the GeoTIFF")
            assert p.stats().points_processed == model.survivors, \
                f"{at}: points_processed {p.stats().points_processed} != {model.survivors} survivors of the filter"
            if case["acc"]:
                check_acc(at)
                check_tables(at)
            if case["poly"]:
                check_point_tables(at)
                check_twins(at)
                for name in case["poly"]["outlines"]:
                    check_outline(at, name)
        elif o["op"] == "set_polygons":                          # a channel's second set, between ingests: maybe right behind an
            set_polygons(p, case["poly"]["names"][o["channel"]], case["poly"]["sets"][o["channel"]][1])     # ingest nobody waited for
            model.current[o["channel"]] = 1
        elif o["op"] == "point_tables":
            check_point_tables(at, o["counts"])
        elif o["op"] == "set_zones_poly":                        # an external entry's labels burnt from a polygon set
            st = case["poly"]["zone_sets"][o["poly"]]
            zname = plan["zonal"][o["zonal"]]["zones"]
            p.set_zones(zname, st["polys"].to_pcr(), background=st["opts"]["background"])
            model.zones[zname] = model.burn(st["polys"], np.float32(st["opts"]["background"]))
        elif o["op"] == "polygonize":
            check_outline(at, o["band"])
        elif o["op"] == "reburn":                                # the twin's zones from the crowns' outlines; refused: nothing is set
            import polygonize_common as PG
            got = check_outline(at, o["band"])
            if got is not None:
                zname = plan["zonal"][o["zonal"]]["zones"]
                p.set_zones(zname, got)
                model.zones[zname] = PG.burn_target(model.finalized[1][model.finalized[0].index(o["band"])])
                model.burnt[o["zonal"]] = model.finalizes
                check_twins(at)
        elif o["op"] == "read_acc":
            check_acc(at)
        elif o["op"] == "tables":
            check_tables(at)
        elif o["op"] == "set_zones":                             # an external label grid; a second set replaces the copy
            import overviews_common as OV
            z = [q for q in plan["zonal"] if q["external"]][o["entry"]]
            labels = external_labels(case["grid"], case["acc"]["labels"][o["entry"]][o["labels"]])
            p.set_zones(z["zones"], OV.make_grid([np.zeros_like(labels), labels]), 1)
            model.zones[z["zones"]] = labels
        elif case["acc"] and o["op"] in ("reload", "checkpoint"):
            # checkpoints do not carry the accumulators: both calls are refused with the message of the first non-empty list,
            # and neither the state nor the next finalize knows of the call (the model does not move).  A polygon case has
            # point_zonal entries too: save_state and load_state of both engines ask histograms, extremes, cell_stats and only
            # then point_zonal, and an accumulator case has one of the first three -- the pinned message stays theirs
            a = case["acc"]
            what = "histograms' cubes" if a["hist"] else "extremes' key planes" if a["ext"] else "cell stats' planes"
            refusal(lambda: (p.load_state if o["op"] == "reload" else p.save_state)(str(tmp_path / f"ck{k}")),
                    f"checkpoints do not carry the {what} yet", at)
            assert not os.path.exists(str(tmp_path / f"ck{k}")), f"{at}: the refused call left files"
        elif o["op"] in ("planes_read", "planes_write"):
            if not in_core_hip:
                continue                                         # (no plane pointers out of core or on the host engine)
            p.synchronize()                                      # the caller's part: the scatters it enqueued itself
            views = {(group, {1: 0, 2: 1, 4: 2, 8: 3}[kind]): ptr for ptr, kind, group in p.state_planes()}
            want = model.state_planes()
            assert set(views) == set(want), f"{at}: planes {sorted(views)} != {sorted(want)}"
            assert p.state_row_count() == H
            for key in sorted(views):
                M.bits_equal(d2h(views[key], (H, W)), want[key], f"{at}, plane {key}")
            if o["op"] == "planes_write":                        # from outside: the rectangle read, the patch added, its rows written back
                r0, c0, h, w = o["rect"]
                ptr = views[(o["group"], o["slot"])]
                for r in range(r0, r0 + h):
                    at_row = ptr + 4 * (r * W + c0)
                    h2d(at_row, d2h(at_row, (w,)) + np.float32(o["value"]))
                model.patch(o)
        elif o["op"] == "flags":
            if not in_core_hip:
                continue
            p.synchronize()
            ptr, tx, ty = p.tile_touched_ptr(readonly=o["readonly"])
            assert (tx, ty) == (model.tx, model.ty) and ptr != 0, at
            got = d2h(ptr, (ty, tx), np.uint32)
            assert np.array_equal(got != 0, model.touched), f"{at}: touched flags differ"
            for r, c in o["extra"]:                              # written through the pointer, as the shard exchange does
                h2d(ptr + 4 * (r * tx + c), np.ones(1, np.uint32))
            model.flag(o["extra"])
        elif o["op"] == "merge":
            if not in_core_hip:
                continue
            model.flag(o["extra"])
            union = A.DeviceBuffer.from_numpy(model.touched.astype(np.uint32))
            alive.append(union)
            p.merge_touched(union.ptr.value)
        elif o["op"] == "reload":                                # an earlier checkpoint laid over the state as it is
            p.load_state(str(tmp_path / f"ck{o['of']}"))
            model.overlay(snaps[o["of"]])
        else:                                                    # checkpoint
            ck = str(tmp_path / f"ck{k}")
            p.save_state(ck)
            # the files a host-engine pipeline writes for the same state
            src, ref = str(tmp_path / f"ck{k}_model"), str(tmp_path / f"ck{k}_host")
            os.makedirs(src)
            model.write_checkpoint(src)
            hcfg = make_config(case, dict(fill=0, ground=None, loc="Host", out=False, cog=False), dict(ooc=False), pcr.ExecutionMode.CPU,
                               "host", tmp_path, src)
            hp = pcr.Pipeline.create(hcfg)
            assert hp is not None and hp.engine() == "host", f"{at}: {pcr.pipeline_create_error()}"
            os.makedirs(ref)
            hp.save_state(ref)
            del hp
            if not os.path.isdir(ck):
                os.makedirs(ck)                                  # (nothing touched: nothing written)
            _same_tree(ck, ref, at)
            snaps[k] = model.snapshot()
            if o["then"] == "go_on":
                continue
            plan, flavour = o["plan"] or plan, o["flavour"] or flavour
            if hip:
                p.synchronize()
            del p
            if o["then"] == "fresh":                             # a new pipeline that does not take the state (a later op may load it)
                model = Model(case)
                p = create()
                continue
            model.carried_over()
            if o["then"] == "resume":
                p = create(ck)
            else:
                p = create()
                p.load_state(ck)
            first_ingest = False
    assert case["ops"][-1]["op"] == "finalize"
    if hip:
        p.synchronize()
    del p
