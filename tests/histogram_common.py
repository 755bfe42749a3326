"""Shared by tests/test_histogram_host.py and tests/test_gpu_histogram.py: the NumPy model of the per-cell histogram contract
(include/pcr_hip.h, "per-cell histograms") -- no engine code: the float64 bin rule one rounded NumPy operation at a time,
np.add.at into the cube, the percentile walk -- and the builders of clouds and configurations.  Every comparison made with it is
np.array_equal on uint32 views: the fold is integer addition, there is no tolerance anywhere."""
import numpy as np

F32, F64 = np.float32, np.float64
NAN_BITS = 0x7FC00000

# the pipeline grid of the tests: 131 x 37 cells of 0.5, four reference tiles across and three down (ragged ones included)
GRID = dict(min_x=10.0, min_y=-3.0, max_x=75.5, max_y=15.5, cs=0.5, W=131, H=37, tw=40, th=16)
PERCENTILES = [0.0, 0.25, 0.5, 0.95, 1.0]
LO, HI = -4.0, 28.0


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def bits_equal(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} differ, first at {bad[:5].tolist()}: got "
                           f"{[hex(v) for v in g.ravel()[bad[:5]]]} want {[hex(v) for v in w.ravel()[bad[:5]]]}")


def cubes_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint32 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} counters differ, first at {bad[:5].tolist()}"


# ---- the model ------------------------------------------------------------------------------------------------------------
def route(g, x, y):
    """The Point glyph's rule: inclusive bounds, floor of the TRUE float64 quotient, clamp.  -> (valid, row, col)"""
    x, y = np.ascontiguousarray(x, F64), np.ascontiguousarray(y, F64)
    with np.errstate(all="ignore"):
        valid = (x >= g["min_x"]) & (x <= g["max_x"]) & (y >= g["min_y"]) & (y <= g["max_y"])
        xs, ys = np.where(valid, x, g["min_x"]), np.where(valid, y, g["max_y"])
        col = np.clip(np.floor((xs - F64(g["min_x"])) / F64(g["cs"])), 0, g["W"] - 1).astype(np.int64)
        row = np.clip(np.floor((ys - F64(g["max_y"])) / F64(-g["cs"])), 0, g["H"] - 1).astype(np.int64)
    return valid, row, col


def bin_of(v, lo, hi, bins):
    """Float64: inv_w once, one subtraction, one multiplication, the clamps.  -1 for a NaN value."""
    v = np.ascontiguousarray(v, F32)
    inv_w = F64(bins) / (F64(F32(hi)) - F64(F32(lo)))
    with np.errstate(all="ignore"):
        t = (v.astype(F64) - F64(F32(lo))) * inv_w
        b = np.where(t < 0, 0, np.where(t >= bins, bins - 1, np.floor(np.where(np.isfinite(t), t, 0.0)))).astype(np.int64)
    return np.where(np.isnan(v), -1, b)


def cube(g, x, y, v, lo, hi, bins, keep=None):
    """count[b][row][col] of the accepted points, uint32."""
    valid, row, col = route(g, x, y)
    b = bin_of(v, lo, hi, bins)
    ok = valid & (b >= 0)
    if keep is not None:
        ok &= np.asarray(keep, bool)
    out = np.zeros((bins, g["H"], g["W"]), np.uint32)
    np.add.at(out, (b[ok], row[ok], col[ok]), 1)
    return out


def percentiles(counts, lo, hi, bins, qs):
    """The bands for qs out of a cube (bins, H, W): the walk of the contract, every operation rounded on its own."""
    counts = np.asarray(counts, np.uint32)
    lo64 = F64(F32(lo))
    w = (F64(F32(hi)) - lo64) / bins
    c64 = counts.astype(np.int64)
    total = c64.sum(axis=0)
    cum = np.cumsum(c64, axis=0)
    out = []
    for q in qs:
        with np.errstate(all="ignore"):
            k = np.ceil(F64(F32(q)) * total.astype(F64)).astype(np.int64)
            k = np.minimum(np.maximum(k, 1), np.maximum(total, 1))
            b = np.argmax(cum >= k[None], axis=0)                                     # the smallest bin with C_b >= k
            below = np.where(b > 0, np.take_along_axis(cum, np.maximum(b - 1, 0)[None], axis=0)[0], 0)
            in_bin = np.take_along_axis(c64, b[None], axis=0)[0]
            pos = ((k - below).astype(F64) - F64(0.5)) / np.maximum(in_bin, 1).astype(F64)
            off = w * (b.astype(F64) + pos)
            band = (lo64 + off).astype(F32)
        band.view(np.uint32)[total == 0] = NAN_BITS
        out.append(band)
    return out


def band_name(channel, q):
    return f"{channel}_p{int(np.floor(float(F32(q)) * 100.0 + 0.5))}"


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def make_points(n, seed, g=GRID, lo=LO, hi=HI, bins=37, hot=0.6):
    """n points: `hot` of them in ONE cell, the rest over and a little beyond the grid, some exactly on the bounds; values
    normal inside [lo, hi) with NaN, +-Inf, values below lo, at and above hi, and values exactly on bin edges among them; cls 1 / 2
    / 5 and ret 1..3 for the filters."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(g["min_x"] - 2.0, g["max_x"] + 2.0, n)
    y = rng.uniform(g["min_y"] - 2.0, g["max_y"] + 2.0, n)
    nh = int(n * hot)
    hot_col, hot_row = g["W"] // 3, g["H"] // 2
    x[:nh] = g["min_x"] + (hot_col + rng.uniform(0.05, 0.95, nh)) * g["cs"]
    y[:nh] = g["max_y"] - (hot_row + rng.uniform(0.05, 0.95, nh)) * g["cs"]
    edge = rng.choice(np.arange(nh, n), 64, replace=False)                 # exactly on the bounds: inclusive
    x[edge[:16]], x[edge[16:32]] = g["min_x"], g["max_x"]
    y[edge[32:48]], y[edge[48:]] = g["min_y"], g["max_y"]
    v = (rng.standard_normal(n) * (hi - lo) / 6.0 + (hi + lo) / 2.0).astype(F32)
    odd = rng.permutation(n)
    k = max(n // 50, 8)
    v[odd[0:k]] = np.nan
    v[odd[k:2 * k]] = np.inf
    v[odd[2 * k:3 * k]] = -np.inf
    v[odd[3 * k:4 * k]] = F32(lo) - rng.uniform(0.0, 100.0, k).astype(F32)       # below lo (and lo itself is an edge below)
    v[odd[4 * k:5 * k]] = F32(hi) + rng.uniform(0.0, 100.0, k).astype(F32)       # above hi
    v[odd[5 * k:5 * k + 4]] = F32(hi)                                           # at hi: the last bin
    on_edge = odd[6 * k:9 * k]                                                  # exactly on bin edges, lo included
    v[on_edge] = (F64(lo) + rng.integers(0, bins, on_edge.size) * ((F64(hi) - F64(lo)) / bins)).astype(F32)
    order = rng.permutation(n)                                                  # the hot cell's points anywhere in the cloud
    return dict(x=x[order], y=y[order], z=v[order], cls=rng.choice(np.array([1, 2, 5], F32), n),
                ret=rng.integers(1, 4, n).astype(F32))


def take(c, idx):
    return {k: a[idx] for k, a in c.items()}


def uneven_splits(n, parts, seed):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), parts - 1, replace=False))
    return [np.arange(a, b) for a, b in zip(np.r_[0, cuts], np.r_[cuts, n])]


def make_cloud(pcr, c, location=None):
    n = len(c["x"])
    cloud = pcr.PointCloud.create(max(n, 1))
    cloud.set_x_array(np.ascontiguousarray(c["x"], F64))
    cloud.set_y_array(np.ascontiguousarray(c["y"], F64))
    for name, a in c.items():
        if name in ("x", "y"):
            continue
        cloud.add_channel(name, pcr.DataType.Float32)
        cloud.set_channel_array_f32(name, np.ascontiguousarray(a, F32))
    return cloud.to_device() if location is not None and location == pcr.MemoryLocation.Device else cloud


# ---- configurations -------------------------------------------------------------------------------------------------------
def histogram(pcr, channel="z", lo=LO, hi=HI, bins=37, qs=PERCENTILES, names=(), filt=()):
    h = pcr.HistogramConfig(channel, lo, hi, bins, [float(q) for q in qs])
    h.band_names = list(names)
    if filt:
        f = pcr.FilterSpec()
        for ch, op, val in filt:
            f.add(ch, getattr(pcr.CompareOp, op), float(val))
        h.filter = f
    return h


def make_config(pcr, mode, histograms, g=GRID, reductions=(("z", "Max"), ("z", "Min")), cfg_filt=(), **kw):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(g["min_x"], g["min_y"], g["max_x"], g["max_y"])
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = g["cs"], -g["cs"]
    cfg.grid.tile_width, cfg.grid.tile_height = g["tw"], g["th"]
    cfg.grid.compute_dimensions()
    assert (cfg.grid.width, cfg.grid.height) == (g["W"], g["H"])
    cfg.exec_mode = pcr.ExecutionMode.CPU if mode == "cpu" else pcr.ExecutionMode.GPU
    specs = []
    for ch, t in reductions:
        r = pcr.ReductionSpec()
        r.value_channel, r.type = ch, getattr(pcr.ReductionType, t)
        specs.append(r)
    cfg.reductions = specs
    if cfg_filt:
        f = pcr.FilterSpec()
        for ch, op, val in cfg_filt:
            f.add(ch, getattr(pcr.CompareOp, op), float(val))
        cfg.filter = f
    cfg.histograms = list(histograms)
    for k, val in kw.items():
        setattr(cfg, k, val)
    return cfg


def keep_mask(c, preds):
    """AND of simple predicates [(channel, op name, value)] over a cloud dict, as float32 comparisons."""
    ops = {"Equal": np.equal, "NotEqual": np.not_equal, "Less": np.less, "LessEqual": np.less_equal, "Greater": np.greater,
           "GreaterEqual": np.greater_equal}
    keep = np.ones(len(c["x"]), bool)
    with np.errstate(all="ignore"):
        for ch, op, val in preds:
            keep &= ops[op](np.asarray(c[ch], F32), F32(val))
    return keep


def result_bands(p):
    res = p.result()
    res = res.to_host() if res.location() != type(res.location()).Host else res
    names = [res.band_desc(b).name for b in range(res.num_bands())]
    return names, [np.array(res.band_array(b)) for b in range(res.num_bands())]
