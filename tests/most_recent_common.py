"""What the MostRecent tests share: the NumPy model of the contract (include/pcr_hip.h "MostRecent"), a literal loop of the
reference's combine_timestamped, cell routing, and bitwise band comparison.  No engine code is used here."""
import numpy as np

import pcr
import pcr_oracle_py as O

FLT_MAX = np.float32(3.4028234663852886e38)
EMPTY_VALUE_BITS = np.uint32(0x7FC00000)


def ord32(f):
    """Float bits -> unsigned integers, monotonically: b ^ (sign ? 0xFFFFFFFF : 0x80000000)."""
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unord32(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.where(u >> np.uint32(31), u ^ np.uint32(0x80000000), ~u).astype(np.uint32).view(np.float32)


def word(t, v):
    """word(t, v) = ord(t + 0.0f) << 32 | ord(v)."""
    t = np.asarray(t, dtype=np.float32) + np.float32(0.0)
    return (ord32(t).astype(np.uint64) << np.uint64(32)) | ord32(v).astype(np.uint64)


def accepted(t):
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (t == t) & (t > -FLT_MAX)


def cells_oracle(og, x, y):
    """Flat cell index of every point by the frozen oracle's world_to_cell, -1 outside the bounds (small clouds)."""
    out = np.full(len(x), -1, dtype=np.int64)
    for i in range(len(x)):
        c, r, ok = O.world_to_cell(og, float(x[i]), float(y[i]))
        if ok:
            out[i] = r * og.width + c
    return out


def cells_floor(x, y, W, H):
    """Interior points of a north-up unit-cell grid with bounds (0, 0, W, H): col = floor(x), row = floor(H - y)."""
    return (np.floor(H - y).astype(np.int64) * W + np.floor(x).astype(np.int64))


def fold_words(cell, v, t, ncells, keep=None, words=None):
    """The state: per cell the maximum word of its accepted points, 0 where it has none."""
    if words is None:
        words = np.zeros(ncells, dtype=np.uint64)
    ok = (cell >= 0) & accepted(t)
    if keep is not None:
        ok &= keep
    np.maximum.at(words, cell[ok], word(np.asarray(t)[ok], np.asarray(v)[ok]))
    return words


def band_of_words(words, shape, touched_cells=None):
    """The band: the value where the word is non-zero, NaN elsewhere."""
    out = np.full(words.shape, np.nan, dtype=np.float32)
    m = words != 0
    out[m] = unord32((words[m] & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    return out.reshape(shape)


def state_of_words(words, shape):
    """The two float planes at the boundary: {value, timestamp}, an empty cell {NaN 0x7FC00000, -FLT_MAX}."""
    val = np.full(words.shape, EMPTY_VALUE_BITS, dtype=np.uint32).view(np.float32).copy()
    ts = np.full(words.shape, -FLT_MAX, dtype=np.float32)
    m = words != 0
    val[m] = unord32((words[m] & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    ts[m] = unord32((words[m] >> np.uint64(32)).astype(np.uint32))
    return val.reshape(shape), ts.reshape(shape)


def model_band(cell, v, t, shape, keep=None):
    return band_of_words(fold_words(cell, v, t, shape[0] * shape[1], keep), shape)


def reference_loop(cell, v, t, shape, order):
    """MostRecentOp (include/pcr/ops/builtin_ops.h:109-124 of the reference), literally: identity {NaN, -FLT_MAX},
    combine_timestamped `ts > acc.timestamp ? {val, ts} : acc`, finalize = acc.value; points visited in `order`."""
    value = np.full(shape[0] * shape[1], np.nan, dtype=np.float32)
    stamp = np.full(shape[0] * shape[1], -FLT_MAX, dtype=np.float32)
    v = np.asarray(v, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    for i in order:
        c = cell[i]
        if c < 0:
            continue
        if t[i] > stamp[c]:
            value[c], stamp[c] = v[i], t[i]
    return value.reshape(shape)


def assert_bits(got, want, what=""):
    """Bitwise on view(uint32) outside the NaN cells, the NaN masks equal."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN mask differs in {int((gn != wn).sum())} cells, first {np.argwhere(gn != wn)[:3].tolist()}"
    g, w = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} cells differ bitwise"


def make_cfg(W, H=None, tile=None, mode=None, threads=0):
    H = H or W
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    if tile:
        cfg.grid.tile_width, cfg.grid.tile_height = tile
    cfg.grid.compute_dimensions()
    cfg.exec_mode = mode if mode is not None else pcr.ExecutionMode.CPU
    cfg.cpu_threads = threads
    return cfg


def oracle_grid(W, H=None, tile=None):
    H = H or W
    return O.make_grid((0.0, 0.0, float(W), float(H)), tile=tile or (4096, 4096))


def make_cloud(x, y, **channels):
    cloud = pcr.PointCloud.create(len(x))
    cloud.set_x_array(np.asarray(x, dtype=np.float64))
    cloud.set_y_array(np.asarray(y, dtype=np.float64))
    for name, arr in channels.items():
        cloud.add_channel(name, pcr.DataType.Float32)
        cloud.set_channel_array_f32(name, np.asarray(arr, dtype=np.float32))
    return cloud


def most_recent_spec(value="value", stamp="time"):
    r = pcr.ReductionSpec()
    r.value_channel, r.type, r.timestamp_channel = value, pcr.ReductionType.MostRecent, stamp
    return r


def spec(rtype, value="value"):
    r = pcr.ReductionSpec()
    r.value_channel, r.type = value, rtype
    return r


def bands(pipe):
    res = pipe.result()
    return [np.array(res.band_array(b)) for b in range(res.num_bands())]


def tricky_cloud(W, H, n, seed, stamps="mixed"):
    """Points on the bounds (Q1: inclusive), outside them, and timestamps the acceptance rule must judge."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.0, W + 3.0, n)
    y = rng.uniform(-3.0, H + 3.0, n)
    k = n // 10
    x[:k] = rng.choice([0.0, float(W)], k)                       # on the left / right bound
    y[k:2 * k] = rng.choice([0.0, float(H)], k)                  # on the bottom / top bound
    v = rng.normal(0.0, 100.0, n).astype(np.float32)
    v[rng.integers(0, n, n // 50)] = np.nan                      # a NaN value is copied like any other
    v[rng.integers(0, n, n // 50)] = np.float32(-0.0)
    if stamps == "ties":
        t = rng.integers(0, 8, n).astype(np.float32)
    else:
        t = rng.uniform(-1e6, 1e6, n).astype(np.float32)
        special = np.array([np.nan, -np.inf, -FLT_MAX, np.inf, 0.0, -0.0, FLT_MAX, -1e-45, 1e-45], dtype=np.float32)
        idx = rng.integers(0, n, n // 4)
        t[idx] = special[rng.integers(0, len(special), len(idx))]
    return x, y, v, t
