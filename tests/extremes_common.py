"""Shared by tests/test_extremes_host.py and tests/test_gpu_extremes.py: the NumPy model of the per-cell extremes contract
(include/pcr_hip.h, "per-cell extremes") -- no engine code: the key on the bits, np.unique of every cell's keys cut to the first k,
the band walk in np.float32 -- and the builders of clouds and configurations.  Every comparison made with it is np.array_equal on
uint32 views: the state is a set of keys, there is no tolerance anywhere."""
import numpy as np

import histogram_common as H

F32, F64 = np.float32, np.float64
NAN_BITS = 0x7FC00000
EMPTY = np.uint32(0xFFFFFFFF)
LOWEST, HIGHEST = 0, 1

# the pipeline grid of the tests: 33 x 19 cells of 0.5, three reference tiles across and three down (ragged ones included); small,
# so that most cells see more than k distinct values
GRID = dict(min_x=10.0, min_y=-3.0, max_x=26.5, max_y=6.5, cs=0.5, W=33, H=19, tw=16, th=8)
bits, bits_equal, route, take, uneven_splits, make_cloud, keep_mask, result_bands = (
    H.bits, H.bits_equal, H.route, H.take, H.uneven_splits, H.make_cloud, H.keep_mask, H.result_bands)


def keys_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint32 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} keys differ, first at {bad[:5].tolist()}: got "
                               f"{[hex(v) for v in got[tuple(bad[:5].T)]]} want {[hex(v) for v in want[tuple(bad[:5].T)]]}")


# ---- the model ------------------------------------------------------------------------------------------------------------
def key_of(v, side):
    """Bits of v, -0.0 folded to +0.0 on the bits, ord() for LOWEST, ~ord() for HIGHEST; EMPTY for a NaN."""
    b = np.ascontiguousarray(v, F32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    o = b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    k = ~o if side == HIGHEST else o
    return np.where(np.isnan(np.ascontiguousarray(v, F32)), EMPTY, k).astype(np.uint32)


def value_of(keys, side):
    """The decoded floats; NaN (0x7FC00000) for EMPTY."""
    keys = np.asarray(keys, np.uint32)
    o = ~keys if side == HIGHEST else keys
    b = np.where(o >> 31 != 0, o ^ np.uint32(0x80000000), ~o).astype(np.uint32)
    b[keys == EMPTY] = NAN_BITS
    return b.view(F32)


def planes(g, x, y, v, k, side, keep=None):
    """keys[j][row][col]: per cell, np.unique of the accepted points' keys, the first k of them; EMPTY behind."""
    valid, row, col = route(g, x, y)
    key = key_of(v, side)
    ok = valid & (key != EMPTY)
    if keep is not None:
        ok &= np.asarray(keep, bool)
    out = np.full((k, g["H"], g["W"]), EMPTY, np.uint32)
    pairs = np.unique(((row[ok] * g["W"] + col[ok]).astype(np.uint64) << np.uint64(32)) | key[ok].astype(np.uint64))
    cell, kk = (pairs >> np.uint64(32)).astype(np.int64), (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    at = np.arange(pairs.size)
    start = np.maximum.accumulate(np.where(np.r_[True, cell[1:] != cell[:-1]], at, 0)) if pairs.size else at
    rank = at - start                                                     # the place of the key among its cell's distinct keys
    m = rank < k
    out.reshape(k, -1)[rank[m], cell[m]] = kk[m]
    return out


def band(keys, side, max_gap):
    """The walk of the contract, every subtraction one np.float32 operation.  -> float32 (H, W)"""
    keys = np.asarray(keys, np.uint32)
    k = keys.shape[0]
    v = value_of(keys, side)
    n = (keys != EMPTY).sum(axis=0)
    i = np.zeros(keys.shape[1:], np.int64)
    gap = F32(max_gap)
    with np.errstate(all="ignore"):
        for j in range(1, k):
            d = (v[j - 1] - v[j]) if side == HIGHEST else (v[j] - v[j - 1])
            assert d.dtype == F32
            i[(i == j - 1) & (j < n) & (d > gap)] = j
    out = np.take_along_axis(v, i[None], axis=0)[0].copy()
    out.view(np.uint32)[n == 0] = NAN_BITS
    return out


def band_name(channel, side):
    return channel + ("_high" if side == HIGHEST else "_low")


def fold_zero(a):
    """The bits of a float32 array with -0.0 folded to +0.0: what the key does to a value before it is kept."""
    b = bits(a).copy()
    b[b == 0x80000000] = 0
    return b


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def make_points(n, seed, g=GRID, hot=0.6, shift=0.0):
    """n points: `hot` of them in ONE cell, the rest over and a little beyond the grid, some exactly on the bounds; values
    multiples of 0.25 in [-3, 3] (+ shift) -- duplicates abound, most cells of the small grids see more than k distinct values --
    with NaN, +-Inf, -0.0 and +0.0 among them; cls 1 / 2 / 5 and ret 1..3 for the filters."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(g["min_x"] - 0.5, g["max_x"] + 0.5, n)
    y = rng.uniform(g["min_y"] - 0.5, g["max_y"] + 0.5, n)
    nh = int(n * hot)
    hot_col, hot_row = g["W"] // 3, g["H"] // 2
    x[:nh] = g["min_x"] + (hot_col + rng.uniform(0.05, 0.95, nh)) * g["cs"]
    y[:nh] = g["max_y"] - (hot_row + rng.uniform(0.05, 0.95, nh)) * g["cs"]
    edge = rng.choice(np.arange(nh, n), 64, replace=False)                 # exactly on the bounds: inclusive
    x[edge[:16]], x[edge[16:32]] = g["min_x"], g["max_x"]
    y[edge[32:48]], y[edge[48:]] = g["min_y"], g["max_y"]
    v = (rng.integers(-12, 13, n) * 0.25).astype(F32)
    odd = rng.permutation(n)
    m = max(n // 50, 8)
    v[odd[0:m]] = np.nan
    v[odd[m:m + m // 4]] = np.inf
    v[odd[2 * m:2 * m + m // 4]] = -np.inf
    v[odd[3 * m:4 * m]] = F32(-0.0)
    v[odd[4 * m:5 * m]] = F32(0.0)
    if shift != 0.0:                                                       # (the zeros too; -0.0 + 0.0 would lose its sign)
        v = v + F32(shift)
    order = rng.permutation(n)                                             # the hot cell's points anywhere in the cloud
    return dict(x=x[order], y=y[order], z=v[order], cls=rng.choice(np.array([1, 2, 5], F32), n),
                ret=rng.integers(1, 4, n).astype(F32))


def check_cloud(c, g):
    """What the tests rely on the cloud having."""
    z = c["z"]
    zb = bits(z)
    assert np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any()
    assert (zb == 0x80000000).any() and (zb == 0).any()
    valid, row, col = route(g, c["x"], c["y"])
    assert (~valid).any() and (c["x"] == g["min_x"]).any() and (c["y"] == g["max_y"]).any()
    assert np.bincount(row[valid] * g["W"] + col[valid]).max() >= 0.6 * len(z)


# ---- configurations -------------------------------------------------------------------------------------------------------
def entry(pcr, channel="z", side=LOWEST, k=4, max_gap=1.0, name="", filt=()):
    e = pcr.ExtremesConfig(channel, pcr.ExtremeSide.Highest if side == HIGHEST else pcr.ExtremeSide.Lowest, k, float(max_gap))
    e.band_name = name
    if filt:
        f = pcr.FilterSpec()
        for ch, op, val in filt:
            f.add(ch, getattr(pcr.CompareOp, op), float(val))
        e.filter = f
    return e


def make_config(pcr, mode, extremes, g=GRID, reductions=(("z", "Max"), ("z", "Min")), cfg_filt=(), **kw):
    cfg = H.make_config(pcr, mode, [], g=g, reductions=reductions, cfg_filt=cfg_filt)
    cfg.extremes = list(extremes)
    for k, val in kw.items():
        setattr(cfg, k, val)
    return cfg


# ---- the scenario that shows the point ------------------------------------------------------------------------------------
SCENE = dict(min_x=0.0, min_y=0.0, max_x=64.0, max_y=48.0, cs=1.0, W=64, H=48, tw=32, th=32)


def plane_z(x, y):
    return 100.0 + 0.05 * np.asarray(x, F64) + 0.03 * np.asarray(y, F64)


def make_scene(offset, seed=7, per_cell=12, rate=0.01):
    """A tilted plane (0.08 of relief inside a cell, 4.64 over the grid), per_cell returns in every cell, and `rate` of the returns
    moved by `offset` (-50: multipath pits, +80: birds).  The outliers of one cell -- three at the most, so that k = 4 keeps a true
    return -- lie a further 3 apart each, so that the walk has to step over every one of them.  -> (cloud dict, outlier mask)"""
    g = SCENE
    rng = np.random.default_rng(seed)
    cols, rows = np.meshgrid(np.arange(g["W"]), np.arange(g["H"]))
    col, row = np.repeat(cols.ravel(), per_cell), np.repeat(rows.ravel(), per_cell)
    n = col.size
    x = g["min_x"] + (col + rng.uniform(0.02, 0.98, n)) * g["cs"]
    y = g["max_y"] - (row + rng.uniform(0.02, 0.98, n)) * g["cs"]
    z = plane_z(x, y)
    out = rng.random(n) < rate
    out[:3 * per_cell:4] = True                                            # some cells with three outliers for certain
    cell = row * g["W"] + col
    idx = np.flatnonzero(out)
    rank = np.zeros(n, np.int64)
    seen = {}
    for i in idx:
        rank[i] = seen.get(cell[i], 0)
        seen[cell[i]] = rank[i] + 1
    out &= rank < 3
    z = np.where(out, z + offset + np.sign(offset) * 3.0 * rank, z)
    order = rng.permutation(n)
    return dict(x=x[order], y=y[order], z=z.astype(F32)[order]), out[order]


def check_scene(pcr, make_pipeline, mode="cpu"):
    """make_pipeline(cfg, cloud dict) -> a finalized pipeline; mode: "cpu" the host engine, "gpu" the HIP engine."""
    g = SCENE
    cols, rows = np.meshgrid(np.arange(g["W"]), np.arange(g["H"]))
    lo_z = plane_z(cols, g["max_y"] - (rows + 1.0)).astype(np.float32)   # the plane over a cell: its lowest corner
    hi_z = plane_z(cols + 1.0, g["max_y"] - rows).astype(np.float32)     # ... and its highest
    relief = (float(plane_z(0.0, 0.0)), float(plane_z(g["max_x"], g["max_y"])))
    # pits: 1 % of the returns 50 below the plane
    c, is_out = make_scene(-50.0)
    valid, row, col = route(g, c["x"], c["y"])
    assert valid.all() and 0.005 < is_out.mean() < 0.02
    has_out = np.zeros((g["H"], g["W"]), bool)
    has_out[row[is_out], col[is_out]] = True
    assert np.bincount(row[is_out] * g["W"] + col[is_out]).max() == 3      # up to k - 1 outliers in a cell
    ground = pcr.GroundFilterConfig()
    ground.source_band = "z_low"
    cfg = make_config(pcr, mode, [entry(pcr, "z", LOWEST, 4, 1.0)], g=g, reductions=(("z", "Min"), ("z", "Max")), ground=ground)
    names, bands = result_bands(make_pipeline(cfg, c))
    assert names == ["z_2", "z_1", "z_low", "dtm"]
    zmin, zlow, dtm = bands[0], bands[2], bands[3]
    assert has_out.sum() > 200 and np.array_equal(zmin < lo_z - 40.0, has_out)       # the Min band HAS the pits
    assert ((zlow >= lo_z) & (zlow <= hi_z)).all()                                    # z_low has none: a true return everywhere
    assert np.array_equal(bits(zlow)[~has_out], bits(zmin)[~has_out])             # ... and is the Min where there was no pit
    ok = ~np.isnan(dtm)
    assert ok.mean() > 0.9 and (dtm[ok] >= relief[0]).all() and (dtm[ok] <= relief[1]).all()   # the DTM stays within the plane's relief
    # birds: 1 % of the returns 80 above
    c, is_out = make_scene(80.0, seed=8)
    valid, row, col = route(g, c["x"], c["y"])
    has_out[:] = False
    has_out[row[is_out], col[is_out]] = True
    cfg = make_config(pcr, mode, [entry(pcr, "z", HIGHEST, 4, 1.0)], g=g, reductions=(("z", "Min"), ("z", "Max")))
    names, bands = result_bands(make_pipeline(cfg, c))
    assert names == ["z_2", "z_1", "z_high"]
    zmax, zhigh = bands[1], bands[2]
    assert has_out.sum() > 200 and np.array_equal(zmax > hi_z + 70.0, has_out)       # the Max band takes the birds for the canopy
    assert ((zhigh >= lo_z) & (zhigh <= hi_z)).all()
    assert np.array_equal(bits(zhigh)[~has_out], bits(zmax)[~has_out])
