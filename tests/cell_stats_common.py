"""Shared by tests/test_cell_stats_host.py and tests/test_gpu_cell_stats.py: the model of the per-cell stats contract
(include/pcr_hip.h, "per-cell stats") -- no engine code: the float64 step rule one rounded NumPy operation at a time, np.add.at
into the three integer planes, the bands per non-empty cell with Python ints for D = N * S2 - S1^2 (modulo 2^128, as the
contract's unsigned 128-bit integer) and Python floats, one rounded operation at a time, for the rest -- and the builders of
clouds and configurations, and the pipeline scenarios both engines run.  Every state comparison made with it is np.array_equal on
the integer planes, every band comparison np.array_equal on uint32 views; the one tolerance is check_scene's, derived there."""
import math

import numpy as np

import histogram_common as H

F32, F64 = np.float32, np.float64
NAN_BITS = 0x7FC00000
Q = 1 << 21
MEAN, VARIANCE, STDDEV = 0, 1, 2
SUFFIX = {MEAN: "_mean", VARIANCE: "_var", STDDEV: "_std"}

# the pipeline grid of the tests: 96 x 80 cells of 0.5, three reference tiles across and three down (ragged ones included)
GRID = dict(min_x=10.0, min_y=-3.0, max_x=58.0, max_y=37.0, cs=0.5, W=96, H=80, tw=40, th=32)
bits, bits_equal, route, take, uneven_splits, make_cloud, keep_mask, result_bands = (
    H.bits, H.bits_equal, H.route, H.take, H.uneven_splits, H.make_cloud, H.keep_mask, H.result_bands)


def planes_equal(got, want, what=""):
    for name, g, w, t in zip(("N", "S1", "S2"), got, want, (np.uint32, np.int64, np.uint64)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == t and w.dtype == t and g.shape == w.shape, f"{what}: plane {name}: {g.dtype} {g.shape} against {w.dtype} {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (f"{what}: plane {name}: {bad.shape[0]} cells differ, first at {bad[:5].tolist()}: got "
                                   f"{g[tuple(bad[:5].T)].tolist()} want {w[tuple(bad[:5].T)].tolist()}")


# ---- the model ------------------------------------------------------------------------------------------------------------
def steps(v, origin, res):
    """-> (q int64, counted bool): t = ((double)v - origin) * (1.0 / res), the clamp at -+Q, np.rint (ties to even); a NaN is
    not counted."""
    v = np.ascontiguousarray(v, F32)
    inv_res = F64(1.0) / F64(res)
    with np.errstate(all="ignore"):
        t = (v.astype(F64) - F64(origin)) * inv_res
        q = np.where(t <= -Q, -Q, np.where(t >= Q, Q, np.rint(np.where(np.isfinite(t), t, 0.0)))).astype(np.int64)
    return q, ~np.isnan(v)


def planes(g, x, y, v, origin, res, keep=None, into=None):
    """(N uint32, S1 int64, S2 uint64), each (H, W), of the accepted points; `into`: planes to add to (copied, wrapping)."""
    valid, row, col = route(g, x, y)
    q, counted = steps(v, origin, res)
    ok = valid & counted
    if keep is not None:
        ok &= np.asarray(keep, bool)
    shape = (g["H"], g["W"])
    n, s1, s2 = ((np.zeros(shape, np.uint32), np.zeros(shape, np.int64), np.zeros(shape, np.uint64)) if into is None
                 else tuple(np.array(a) for a in into))
    cell = row[ok] * g["W"] + col[ok]
    with np.errstate(over="ignore"):
        np.add.at(n.reshape(-1), cell, np.uint32(1))
        np.add.at(s1.reshape(-1), cell, q[ok])
        np.add.at(s2.reshape(-1), cell, (q[ok] * q[ok]).astype(np.uint64))
    return n, s1, s2


def cell_bands(n, s1, s2, origin, res, ddof):
    """One cell, Python ints and floats: -> (mean, variance, stddev) as Python floats not yet rounded to binary32, None = NaN."""
    n, s1, s2, origin, res = int(n), int(s1), int(s2), float(origin), float(res)
    if n == 0:
        return None, None, None
    mean = origin + res * (float(s1) / float(n))
    if n <= ddof:
        return mean, None, None
    d = (n * s2 - s1 * s1) % (1 << 128)                                    # the contract's unsigned 128-bit integer
    hi, lo = d >> 64, d & ((1 << 64) - 1)
    dd = float(hi) * 2.0 ** 64 + float(lo)                                 # the two conversions, one product (exact), one sum
    den = float(n) * float(n - ddof)
    vq = dd / den
    return mean, (res * res) * vq, res * math.sqrt(vq)


def bands(n, s1, s2, origin, res, ddof=0):
    """-> {MEAN: band, VARIANCE: band, STDDEV: band}, float32 arrays shaped like n; NaN (0x7FC00000) where the contract says."""
    n, s1, s2 = np.asarray(n, np.uint32), np.asarray(s1, np.int64), np.asarray(s2, np.uint64)
    out = {p: np.full(n.shape, NAN_BITS, np.uint32).view(F32) for p in (MEAN, VARIANCE, STDDEV)}
    flat = {p: out[p].reshape(-1) for p in out}
    fn, f1, f2 = n.reshape(-1), s1.reshape(-1), s2.reshape(-1)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(fn):
            for p, val in zip((MEAN, VARIANCE, STDDEV), cell_bands(fn[i], f1[i], f2[i], origin, res, ddof)):
                if val is not None:
                    flat[p][i] = F32(val)                                  # (float)(...): round to nearest even
    return out


def preset_states():
    """Hand-made states for the band arithmetic, (2, 8) planes; every cell names what it is there for."""
    cells = [
        (0, 0, 0),                                                          # N = 0: NaN everywhere
        (1, 12345, 12345 ** 2),                                             # N = 1: ddof 1 -> NaN spread, a valid mean
        (1, -Q, Q * Q),                                                     # ... at the negative clamp
        (2, 2 * 777, 2 * 777 ** 2),                                         # N = 2, equal values: D = 0
        (2, -3, 5),                                                         # N = 2, values -1 and -2: D = 1
        (3_000_000_000, (1 << 52) + 12345, (1 << 63) + 987654321),          # the issue's literal state: D < 0, i.e. modulo 2^128
        (3_000_000_000, -((1 << 52) + 12345), (1 << 63) + 987654321),
        (3_000_000_000, (1 << 47) + 12345, (1 << 63) + 987654321),          # N * S2 > S1^2 (Cauchy-Schwarz holds), D ~ 2^94: hi != 0
        (3_000_000_000, -((1 << 47) + 12345), (1 << 63) - 987654321),
        (2, 1, (1 << 63) + 3),                                              # D = 2^64 + 5: just above 2^64
        (2, 1, 1 << 63),                                                    # D = 2^64 - 1: hi = 0, lo rounds up to 2^64
        (5, 1 << 33, (1 << 64) - 1),                                        # a borrow: lo(N * S2) < lo(S1^2)
        ((1 << 32) - 1, -(1 << 52), (1 << 64) - 1),                         # the largest N
        (4, 6_000_000, 9_000_000_000_020),                                  # z ~ 1500 m at a 1 mm step, sigma a few steps
        (50, 0, 50),                                                        # sigma exactly one step
        (7, 7 * Q, 7 * Q * Q),                                              # all at the positive clamp: D = 0
    ]
    n = np.array([c[0] for c in cells], np.uint32).reshape(2, 8)
    s1 = np.array([c[1] for c in cells], np.int64).reshape(2, 8)
    s2 = np.array([c[2] for c in cells], np.uint64).reshape(2, 8)
    d = [(int(a) * int(c) - int(b) * int(b)) for a, b, c in cells]
    assert any(v >> 64 for v in d if v > 0) and any(v < 0 for v in d) and (1 << 64) + 5 in d and 0 in d
    return n, s1, s2


def twin_bands(A, n, s1, s2, origin, res, ddof, products, own=None):
    """pcr_hip_cell_stats_bands_host on host arrays.  -> list of float32 (own rows, W), in the order of `products`."""
    import ctypes as C
    L = A.lib()
    h, w = n.shape
    g = A.make_grid((0, 0, w, h), dims=(w, h), tile=(w, h))
    r0, r1 = own if own else (0, h)
    g.own_row0, g.own_row1 = r0, r1
    outs = [np.full((r1 - r0, w), -1.0, F32) for _ in products]
    n, s1, s2 = np.ascontiguousarray(n, np.uint32), np.ascontiguousarray(s1, np.int64), np.ascontiguousarray(s2, np.uint64)
    prods = (C.c_int * len(products))(*products)
    ptrs = (C.c_void_p * len(products))(*[o.ctypes.data for o in outs])
    rc = L.pcr_hip_cell_stats_bands_host(C.byref(g), n.ctypes.data, s1.ctypes.data, s2.ctypes.data, origin, res, ddof, len(products),
                                         prods, ptrs)
    assert rc == 0, L.pcr_hip_last_error()
    return outs


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def make_points(n, seed, g=GRID, origin=-2.0, res=2.0 ** -6, sigma=3.0, hot=0.6):
    """n points: `hot` of them in ONE cell, the rest over and a little beyond the grid, some exactly on the bounds and some exactly
    on cell boundaries; values normal around origin (negative steps abound) with NaN, +-Inf, values beyond -+Q steps, exact
    half-steps of both parities (res is a power of two: they are exact), and -0.0 among them; cls 1 / 2 / 5 and ret 1..3 for
    the filters."""
    assert math.log2(res) == int(math.log2(res))
    rng = np.random.default_rng(seed)
    x = rng.uniform(g["min_x"] - 2.0, g["max_x"] + 2.0, n)
    y = rng.uniform(g["min_y"] - 2.0, g["max_y"] + 2.0, n)
    nh = int(n * hot)
    hot_col, hot_row = g["W"] // 3, g["H"] // 2
    x[:nh] = g["min_x"] + (hot_col + rng.uniform(0.05, 0.95, nh)) * g["cs"]
    y[:nh] = g["max_y"] - (hot_row + rng.uniform(0.05, 0.95, nh)) * g["cs"]
    edge = rng.choice(np.arange(nh, n), 128, replace=False)
    x[edge[:16]], x[edge[16:32]] = g["min_x"], g["max_x"]                   # exactly on the bounds: inclusive
    y[edge[32:48]], y[edge[48:64]] = g["min_y"], g["max_y"]
    x[edge[64:96]] = g["min_x"] + rng.integers(1, g["W"], 32) * g["cs"]     # exactly on a cell boundary
    y[edge[96:]] = g["max_y"] - rng.integers(1, g["H"], 32) * g["cs"]
    v = (origin + rng.standard_normal(n) * sigma).astype(F32)
    odd = rng.permutation(n)
    k = max(n // 50, 16)
    v[odd[0:k]] = np.nan
    v[odd[k:k + k // 4]] = np.inf
    v[odd[2 * k:2 * k + k // 4]] = -np.inf
    far = Q * res
    v[odd[3 * k:3 * k + k // 4]] = F32(origin + far * 1.5)                  # beyond +Q steps
    v[odd[4 * k:4 * k + k // 4]] = F32(origin - far * 1.5)                  # beyond -Q steps
    v[odd[5 * k]], v[odd[5 * k + 1]] = F32(origin + far), F32(origin - far)     # exactly +-Q steps
    j = rng.integers(-200, 200, 2 * k)
    v[odd[6 * k:7 * k]] = (origin + (2 * j[:k] + 0.5) * res).astype(F32)    # half-steps, even below: ties go down ...
    v[odd[7 * k:8 * k]] = (origin + (2 * j[k:] + 1.5) * res).astype(F32)    # ... odd below: ties go up
    v[odd[8 * k:9 * k]] = F32(-0.0)
    order = rng.permutation(n)                                              # the hot cell's points anywhere in the cloud
    return dict(x=x[order], y=y[order], z=v[order], cls=rng.choice(np.array([1, 2, 5], F32), n),
                ret=rng.integers(1, 4, n).astype(F32))


def check_cloud(c, g, origin=-2.0, res=2.0 ** -6):
    """What the tests rely on the cloud having."""
    z = c["z"]
    assert np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any() and (bits(z) == 0x80000000).any()
    with np.errstate(all="ignore"):
        t = (z.astype(F64) - origin) / res
    fin = np.isfinite(t)
    assert (t[fin] > Q).any() and (t[fin] < -Q).any() and (t[fin] == Q).any() and (t[fin] == -Q).any() and (t[fin] < 0).any()
    t = np.where(fin, t, 0.0)
    half = fin & (np.abs(t) < Q) & (t - np.floor(t) == 0.5)
    assert (half & (np.floor(t) % 2 == 0)).any() and (half & (np.floor(t) % 2 == 1)).any()
    valid, row, col = route(g, c["x"], c["y"])
    assert (~valid).any() and (c["x"] == g["min_x"]).any() and (c["y"] == g["max_y"]).any()
    fx = (c["x"] - g["min_x"]) / g["cs"]
    assert (valid & (fx == np.floor(fx)) & (fx > 0) & (fx < g["W"])).any()   # on a cell boundary
    assert np.bincount(row[valid] * g["W"] + col[valid]).max() >= 0.55 * len(z)


# ---- configurations -------------------------------------------------------------------------------------------------------
def entry(pcr, channel="z", origin=0.0, res=0.01, products=(STDDEV,), ddof=0, names=(), filt=()):
    kinds = {MEAN: pcr.CellStat.Mean, VARIANCE: pcr.CellStat.Variance, STDDEV: pcr.CellStat.StdDev}
    e = pcr.CellStatsConfig(channel, origin=float(origin), resolution=float(res), products=[kinds[p] for p in products], ddof=ddof)
    e.band_names = list(names)
    if filt:
        f = pcr.FilterSpec()
        for ch, op, val in filt:
            f.add(ch, getattr(pcr.CompareOp, op), float(val))
        e.filter = f
    return e


def make_config(pcr, mode, cell_stats, g=GRID, reductions=(("z", "Max"), ("z", "Min")), cfg_filt=(), **kw):
    cfg = H.make_config(pcr, mode, [], g=g, reductions=reductions, cfg_filt=cfg_filt)
    cfg.cell_stats = list(cell_stats)
    for k, val in kw.items():
        setattr(cfg, k, val)
    return cfg


ALL = (MEAN, VARIANCE, STDDEV)
# (origin, resolution, products, ddof) of the entries most pipeline tests use: a power-of-two step with every product, the
# default centimetre with the sample spread, a coarse step far from the values
SPECS = [(-2.0, 2.0 ** -6, ALL, 0), (0.0, 0.01, (STDDEV, MEAN), 1), (1.5, 0.125, (VARIANCE,), 0)]


def entries(pcr, channel="z"):
    return [entry(pcr, channel, o, r, p, d, names=[f"e{i}{SUFFIX[k]}" for k in p]) for i, (o, r, p, d) in enumerate(SPECS)]


def spec_names():
    return [f"e{i}{SUFFIX[k]}" for i, (_, _, p, _) in enumerate(SPECS) for k in p]


def check_against_model(p, c, keep=None, what="", channel="z", first_band=2):
    """The states and bands of a finalized pipeline built from entries() against the model of cloud dict c."""
    names, got = result_bands(p)
    assert names[first_band:first_band + len(spec_names())] == spec_names(), names
    b = first_band
    for i, (origin, res, products, ddof) in enumerate(SPECS):
        want = planes(GRID, c["x"], c["y"], c[channel], origin, res, keep)
        planes_equal(p.cell_stats(i), want, f"{what}: state of entry {i}")
        model = bands(*want, origin, res, ddof)
        for k in products:
            bits_equal(got[b], model[k], f"{what}: band {names[b]}")
            b += 1


# ---- the scenario that shows the point ------------------------------------------------------------------------------------
SCENE = dict(min_x=0.0, min_y=0.0, max_x=32.0, max_y=32.0, cs=1.0, W=32, H=32, tw=16, th=16)
SCENE_RES = 0.001


def make_scene(seed=5, per_cell=50):
    """About per_cell returns in every cell, z = 1500 + N(0, 0.1^2) as float32: a flat surface at altitude with a decimetre of
    noise.  -> cloud dict"""
    g = SCENE
    rng = np.random.default_rng(seed)
    n = g["W"] * g["H"] * per_cell
    x, y = rng.uniform(g["min_x"], g["max_x"], n), rng.uniform(g["min_y"], g["max_y"], n)
    z = (1500.0 + rng.standard_normal(n) * 0.1).astype(F32)
    return dict(x=x, y=y, z=z)


def check_scene(pcr, make_pipeline, mode="cpu"):
    """make_pipeline(cfg, cloud dict) -> a finalized pipeline.  The bounds are derived, not measured:
       StdDev  |z_std - np.std(z as float64)| <= resolution / 2 + 1e-6: the standard deviation is a seminorm of the deviations, so
               moving every value by at most half a step moves it by at most half a step; 1e-6 covers the binary32 rounding of a
               result near 0.1 (half an ulp is 3.7e-9) and the binary64 arithmetic.
       Mean    |z_mean - mean64| <= resolution / 2 + ulp32(1500): half a step per value, one binary32 rounding of the result."""
    g, res = SCENE, SCENE_RES
    c = make_scene()
    valid, row, col = route(g, c["x"], c["y"])
    assert valid.all()
    cell = row * g["W"] + col
    count = np.bincount(cell, minlength=g["W"] * g["H"])
    assert count.min() >= 20 and 45 < count.mean() < 55
    z64 = c["z"].astype(F64)
    mean64 = np.bincount(cell, z64, g["W"] * g["H"]) / count
    std64 = np.sqrt(np.bincount(cell, (z64 - mean64[cell]) ** 2, g["W"] * g["H"]) / count)
    some = np.flatnonzero(cell == 17)
    assert abs(std64[17] - np.std(z64[some])) < 1e-12 and abs(mean64[17] - np.mean(z64[some])) < 1e-9
    cfg = make_config(pcr, mode, [entry(pcr, "z", 0.0, res, (STDDEV, MEAN))], g=g, reductions=(("z", "Count"),))
    names, got = result_bands(make_pipeline(cfg, c))
    assert len(names) == 3 and names[1:] == ["z_std", "z_mean"]
    z_std, z_mean = got[1].astype(F64).reshape(-1), got[2].astype(F64).reshape(-1)
    ulp32_1500 = float(np.spacing(F32(1500.0)))
    err_std, err_mean = np.abs(z_std - std64), np.abs(z_mean - mean64)
    print(f"scene: max |z_std - std64| = {err_std.max():.3e} (bound {res / 2 + 1e-6:.3e}), "
          f"max |z_mean - mean64| = {err_mean.max():.3e} (bound {res / 2 + ulp32_1500:.3e})")
    assert (err_std <= res / 2 + 1e-6).all()
    assert (err_mean <= res / 2 + ulp32_1500).all()
    return c, cell, count, std64


def naive_float32_std(c, cell, count):
    """What a float32 Sum(v^2)/N - mean^2 gives for the same cells: NumPy float32 accumulation, as the README argues."""
    cells = count.size
    s1, s2 = np.zeros(cells, F32), np.zeros(cells, F32)
    np.add.at(s1, cell, c["z"])
    np.add.at(s2, cell, c["z"] * c["z"])
    nf = count.astype(F32)
    m = s1 / nf
    var = s2 / nf - m * m
    assert var.dtype == F32
    return np.sqrt(np.maximum(var, F32(0.0))).astype(F64)


# ---- the pipeline scenarios both engines run ---------------------------------------------------------------------------------
# run(cfg, clouds, **kw) -> a pipeline of the engine under test with the cloud dicts ingested, not finalized.
N_POINTS = 20_000


def pipeline_points():
    c = make_points(N_POINTS, 11)
    check_cloud(c, GRID)
    return c


def scenario_model_and_splits(pcr, mode, run, c):
    """Bands and states against the model; one ingest equals three chunks equals the reversed cloud; the state is readable before
    any finalize; a filtered entry stands beside the unfiltered ones under PipelineConfig::filter."""
    cfg_filt, own = [("cls", "NotEqual", 5.0)], [("cls", "Equal", 2.0)]
    def ents():
        return entries(pcr) + [entry(pcr, "z", 0.0, 0.01, (MEAN, STDDEV), names=["ground_mean", "ground_std"], filt=own)]
    n = len(c["x"])
    whole = run(make_config(pcr, mode, ents(), cfg_filt=cfg_filt), [c])
    keep = keep_mask(c, cfg_filt)
    origin, res = SPECS[0][:2]
    planes_equal(whole.cell_stats(0), planes(GRID, c["x"], c["y"], c["z"], origin, res, keep), "before any finalize")
    split = run(make_config(pcr, mode, ents(), cfg_filt=cfg_filt), [take(c, i) for i in uneven_splits(n, 3, 5)] + [take(c, np.arange(0))])
    back = run(make_config(pcr, mode, ents(), cfg_filt=cfg_filt), [take(c, np.arange(n)[::-1])])
    for p in (whole, split, back):
        p.finalize()
    check_against_model(whole, c, keep, "one ingest")
    names, ref = result_bands(whole)
    assert names == ["z_1", "z_2"] + spec_names() + ["ground_mean", "ground_std"]
    both = keep & keep_mask(c, own)
    assert 0 < both.sum() < keep.sum()
    want = planes(GRID, c["x"], c["y"], c["z"], 0.0, 0.01, both)
    planes_equal(whole.cell_stats(3), want, "filtered entry: state")
    model = bands(*want, 0.0, 0.01, 0)
    bits_equal(ref[-2], model[MEAN], "filtered entry: mean")
    bits_equal(ref[-1], model[STDDEV], "filtered entry: stddev")
    assert (whole.cell_stats(3)[0] < whole.cell_stats(1)[0]).any()
    for p, what in ((split, "three chunks"), (back, "reversed")):
        for i in range(4):
            planes_equal(p.cell_stats(i), whole.cell_stats(i), f"{what}: state {i}")
        for b, (u, w) in enumerate(zip(result_bands(p)[1][2:], ref[2:])):
            bits_equal(u, w, f"{what}: band {names[2 + b]}")
    return whole


def scenario_surface_channel(pcr, mode, run, c):
    import sample_grid_common as S
    c = dict(c)
    surf = S.Surface(np.random.default_rng(2).integers(-3, 4, (50, 70)).astype(F32), GRID["min_x"] + 1.0, GRID["max_y"] - 1.0, 0.9, -0.8)
    surf.band[3, 5] = np.nan
    own = [("ret", "LessEqual", 2.0), ("hag", "Greater", -2.5)]
    cfg = make_config(pcr, mode, [entry(pcr, "hag", 0.0, 0.01, (MEAN, STDDEV), filt=own)],
                      surface_channels=[pcr.SurfaceChannelConfig("hag", "z", pcr.SampleMode.Bilinear)])
    p = run(cfg, [])
    p.set_surface("hag", S.pcr_grid(pcr, surf))
    p.ingest(make_cloud(pcr, c))
    p.finalize()
    c["hag"] = S.model(surf, c["x"], c["y"], c["z"], S.BILINEAR)          # the model's own sampled channel
    keep = keep_mask(c, own)
    assert 0 < keep.sum() < len(c["x"]) and np.isnan(c["hag"]).sum() > np.isnan(c["z"]).sum()
    want = planes(GRID, c["x"], c["y"], c["hag"], 0.0, 0.01, keep)
    planes_equal(p.cell_stats(0), want, "hag: state")
    names, got = result_bands(p)
    assert names[2:] == ["hag_mean", "hag_std"]
    model = bands(*want, 0.0, 0.01, 0)
    bits_equal(got[2], model[MEAN], "hag: mean")
    bits_equal(got[3], model[STDDEV], "hag: stddev")


def scenario_band_order_fill_and_terrain(pcr, mode, run, c):
    """Band order against percentile, extremes, dtm and terrain bands; terrain on "z_mean"; with fill_nodata_radius = 2 the Mean
    band has fewer NaN cells than raw and the StdDev band is bit-identical to the unfilled run's."""
    import extremes_common as E
    c = take(c, np.arange(0, len(c["x"]), 7))                             # sparse: empty cells to fill
    c["z"] = np.where(np.isfinite(c["z"]) | np.isnan(c["z"]), c["z"], F32(0.5)).astype(F32)

    def cfg(**kw):
        ground = pcr.GroundFilterConfig()
        ground.source_band, ground.max_radius_cells = "z_mean", 2
        t = pcr.TerrainBandConfig()
        t.source_band, t.product = "z_mean", pcr.TerrainProduct.Roughness
        out = make_config(pcr, mode, [entry(pcr, "z", 0.0, 0.01, (MEAN, STDDEV, VARIANCE))], ground=ground, terrain=[t], **kw)
        out.histograms = [H.histogram(pcr, bins=8, qs=[0.5], names=["median"])]
        out.extremes = [E.entry(pcr, "z", E.LOWEST, 2, 1.0)]
        return out
    raw = run(cfg(), [c])
    filled = run(cfg(fill_nodata_radius=2), [c])
    raw.finalize()
    filled.finalize()
    names, got = result_bands(filled)
    assert names == ["z_1", "z_2", "median", "z_low", "z_mean", "z_std", "z_var", "dtm", "z_mean_roughness"]
    raw_names, raw_got = result_bands(raw)
    assert raw_names == names
    model = bands(*planes(GRID, c["x"], c["y"], c["z"], 0.0, 0.01), 0.0, 0.01, 0)
    for b, k in ((4, MEAN), (5, STDDEV), (6, VARIANCE)):
        bits_equal(raw_got[b], model[k], f"raw band {names[b]}")
    assert np.isnan(raw_got[4]).any() and np.isnan(got[4]).sum() < np.isnan(raw_got[4]).sum()      # Mean: filled like an Average band
    m = ~np.isnan(raw_got[4])
    assert np.array_equal(bits(got[4])[m], bits(raw_got[4])[m])                                    # ... the measured cells stay
    bits_equal(got[5], raw_got[5], "StdDev is never filled")
    bits_equal(got[6], raw_got[6], "Variance is never filled")
    assert (~np.isnan(got[7])).any() and (~np.isnan(got[8])).any()                                 # the DTM and the terrain band read z_mean
    return names, got


def refused(pcr, mode, cell_stats, match, **kw):
    assert pcr.Pipeline.create(make_config(pcr, mode, cell_stats, **kw)) is None
    assert match in pcr.pipeline_create_error(), pcr.pipeline_create_error()


def scenario_refusals(pcr, mode):
    e = lambda **kw: entry(pcr, **kw)
    no = lambda cs, match, **kw: refused(pcr, mode, cs, match, **kw)
    no([e(names=[f"b{j}"]) for j in range(5)], "more than 4 cell_stats entries")
    no([e(channel="")], "value_channel is empty")
    for bad in (0.0, -0.01, float("inf"), float("nan"), 1e-320):
        no([e(res=bad)], "resolution must be finite and positive")
    for bad in (float("inf"), float("nan")):
        no([e(origin=bad)], "origin must be finite")
    no([e(products=())], "products must name between 1 and 3 bands")
    no([e(products=(MEAN, VARIANCE, STDDEV, MEAN))], "products must name between 1 and 3 bands")
    no([e(products=(MEAN, MEAN))], "products names a band twice")
    for bad in (-1, 2):
        no([e(ddof=bad)], "ddof must be 0 or 1")
    no([e(names=["a", "b"])], "band_names is longer than products")
    no([e(names=["z_1"])], "collides with another band")                                      # a reduction's band
    no([e(), e()], "collides with another band")                                              # its own twin
    ground = pcr.GroundFilterConfig()
    ground.source_band = "z_2"
    no([e(names=["dtm"])], "collides with another band", ground=ground)
    t = pcr.TerrainBandConfig()
    t.source_band, t.product, t.band_name = "z_2", pcr.TerrainProduct.Hillshade, "shade"
    no([e(names=["shade"])], "collides with another band", terrain=[t])
    import extremes_common as E
    cfg = make_config(pcr, mode, [e(names=["median"])])
    cfg.histograms = [H.histogram(pcr, bins=8, qs=[0.5], names=["median"])]
    assert pcr.Pipeline.create(cfg) is None and "collides with another band" in pcr.pipeline_create_error()
    cfg = make_config(pcr, mode, [e(names=["z_low"])])
    cfg.extremes = [E.entry(pcr)]
    assert pcr.Pipeline.create(cfg) is None and "collides with another band" in pcr.pipeline_create_error()
    no([e()], "cell_stats are not supported on a row-block shard", shard_row_begin=0, shard_row_end=16)


def scenario_checkpoints_refused(pcr, mode, run, c, tmp_path):
    import pytest
    p = run(make_config(pcr, mode, [entry(pcr)]), [c])
    for call in (p.save_state, p.load_state):
        with pytest.raises(RuntimeError, match="checkpoints do not carry the cell stats"):
            call(str(tmp_path))


def scenario_ingest_file(pcr, mode, run, tmp_path):
    """ingest_file of a small LAS tile whose intensity only the cell-stats entry names."""
    import las_common as LC
    fmt, n = 1, 6000
    rng = np.random.default_rng(9)
    f = LC.make_fields(fmt, n, rng)
    f["X"] = rng.integers(-500, 49_000, n).astype(np.int32)
    f["Y"] = rng.integers(-500, 41_000, n).astype(np.int32)
    f["Z"] = rng.integers(-100, 300, n).astype(np.int32)
    scale, offset = (0.001, 0.001, 0.125), (GRID["min_x"], GRID["min_y"], 0.0)
    path = str(tmp_path / "tile.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset)
    want = LC.expected(fmt, f, scale, offset, 0.0)
    cfg = make_config(pcr, mode, [entry(pcr, "intensity", 0.0, 1.0, (MEAN, STDDEV), ddof=1)], reductions=(("z", "Count"), ("z", "Max")))
    p = run(cfg, [])
    assert p.ingest_file(path, 2500) == n
    p.finalize()
    state = planes(GRID, want["x"], want["y"], want["intensity"], 0.0, 1.0)
    planes_equal(p.cell_stats(0), state, "ingest_file: state")
    names, got = result_bands(p)
    assert names[2:] == ["intensity_mean", "intensity_std"]
    model = bands(*state, 0.0, 1.0, 1)
    bits_equal(got[2], model[MEAN], "ingest_file: mean")
    bits_equal(got[3], model[STDDEV], "ingest_file: stddev")
    assert (state[0] > 1).sum() > 100 and (~np.isnan(got[3])).sum() > 100
