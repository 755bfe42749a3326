"""Shared by tests/test_ground_filter.py and tests/test_gpu_ground_filter*.py: the NumPy model of the ground filter (the contract
of csrc/ground_filter.hpp) -- no engine code: the schedule in binary64, erosion and dilation as literal loops over the window,
the level loop on float32 arrays -- and the pipelines' common ground."""
import numpy as np

import overviews_common as M
import pcr

NAN_BITS = M.NAN_BITS
make_grid, grid_bands, values = M.make_grid, M.grid_bands, M.values


def bits_equal(got, want, what=""):
    """Equal NaN masks, equal bits everywhere else."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), f"{what}: NaN masks differ in {int((gn != wn).sum())} cells, first at {np.argwhere(gn != wn)[:3].tolist()}"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~gn
    assert not bad.any(), (f"{what}: {int(bad.sum())} cells differ bitwise, first at {np.argwhere(bad)[:3].tolist()}: "
                           f"{got.view(np.uint32)[bad][:3]} != {want.view(np.uint32)[bad][:3]}")


# ---- the schedule ------------------------------------------------------------------------------------------------------------
def levels(max_radius_cells=16, exponential=True, slope=1.0, initial_distance=0.15, max_distance=2.5, cell=1.0):
    """(radii, thresholds): the spec's fields are binary32, the arithmetic binary64 in the contract's order, rounded once."""
    slope, init, maxd = (float(np.float32(x)) for x in (slope, initial_distance, max_distance))
    radii, thresholds, R, prev = [], [], 1, 0
    while R <= max_radius_cells:
        t = init if not prev else init + slope * float(cell) * 2.0 * float(R - prev)
        radii.append(R)
        thresholds.append(np.float32(min(maxd, t)))
        prev, R = R, (2 * R if exponential else R + 1)
    return radii, thresholds


def spec(**kw):
    s = pcr.GroundFilterSpec()
    for k, v in kw.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    return s


# ---- the filter ---------------------------------------------------------------------------------------------------------------
def _fmin(a, b):
    """minNum spelled out (np.fmin's vector paths do not all ignore a SIGNALLING NaN operand): a NaN operand is ignored."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b < a, b, a)))


def _fmax(a, b):
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b > a, b, a)))


def _window(a, R, pick):
    """pick = _fmin / _fmax over the (2R + 1)^2 window clipped to the image."""
    h, w = a.shape
    p = np.full((h + 2 * R, w + 2 * R), np.nan, np.float32)
    p[R:R + h, R:R + w] = a
    out = np.full((h, w), np.nan, np.float32)
    for dr in range(2 * R + 1):
        if dr + h <= R or dr >= R + h:            # the rows of this offset are all outside the image
            continue
        for dc in range(2 * R + 1):
            if dc + w <= R or dc >= R + w:
                continue
            out = pick(out, p[dr:dr + h, dc:dc + w])
    return out


def erode(a, R):
    return _window(a, R, _fmin)


def dilate(a, R):
    return _window(a, R, _fmax)


def ground_filter(src, radii, thresholds):
    src = np.ascontiguousarray(src, np.float32)
    a = src.copy()
    ground = ~np.isnan(src)
    with np.errstate(all="ignore"):
        for R, t in zip(radii, thresholds):
            o = dilate(erode(a, R), R)
            d = a - o                              # float32 arrays: one binary32 subtraction
            assert d.dtype == np.float32
            ground &= ~(d > np.float32(t))         # a NaN difference compares false
            a = o
    out = np.empty(src.shape, np.float32)
    out.view(np.uint32)[...] = NAN_BITS
    out[ground] = src[ground]
    return out


def difference(top, gnd):
    with np.errstate(all="ignore"):
        d = np.ascontiguousarray(top, np.float32) - np.ascontiguousarray(gnd, np.float32)
    d.view(np.uint32)[np.isnan(d)] = NAN_BITS
    return d


def terrain(w, h, seed, nan_fraction=0.2):
    """A sloping surface with boxes on it (buildings) and empty cells: values a filter has something to say about."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    z = (10.0 + 0.01 * xx + 0.02 * yy + rng.normal(0.0, 0.02, (h, w))).astype(np.float32)
    for _ in range(max(1, w * h // 800)):
        r, c = rng.integers(0, h), rng.integers(0, w)
        z[r:r + rng.integers(1, 12), c:c + rng.integers(1, 12)] += np.float32(rng.uniform(1.0, 8.0))
    z[rng.random((h, w)) < nan_fraction] = np.nan
    return z


# ---- the pipelines' common ground ----------------------------------------------------------------------------------------------
BANDS = ("value_2", "value_1", "value_5")          # Min, Max, Count of pipeline_cfg, as default_band_name names them


def pipeline_cfg(W, H, mode, ground=True, top=True, radius=0, **spec_kw):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    assert (cfg.grid.width, cfg.grid.height) == (W, H)
    cfg.exec_mode = mode
    specs = []
    for t in (pcr.ReductionType.Min, pcr.ReductionType.Max, pcr.ReductionType.Count):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", t
        specs.append(r)
    cfg.reductions = specs
    cfg.fill_nodata_radius = radius
    if ground:
        cfg.ground.source_band = BANDS[0]
        if top:
            cfg.ground.top_band = BANDS[1]
        for k, v in spec_kw.items():
            assert hasattr(cfg.ground, k), k
            setattr(cfg.ground, k, v)
    return cfg


def cloud(W, H, n, seed):
    """Points on a sloping ground with a few raised boxes; the right tenth of the grid stays empty."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0.0, W * 0.9, n), rng.uniform(0.0, H, n)
    z = 10.0 + 0.01 * x + 0.02 * y + rng.normal(0.0, 0.03, n)
    for _ in range(6):
        bx, by, s = rng.uniform(0, W * 0.8), rng.uniform(0, H * 0.9), rng.uniform(3.0, 0.12 * min(W, H) + 3.0)
        inside = (x >= bx) & (x < bx + s) & (y >= by) & (y < by + s)
        z[inside] += rng.uniform(2.0, 9.0)
    c = pcr.PointCloud.create(n)
    c.set_x_array(x)
    c.set_y_array(y)
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", z.astype(np.float32))
    return c


def expect(raw, cfg):
    """What a pipeline with `cfg` returns, from the raw bands [Min, Max, Count] of the same pipeline without ground and
    fill: the host twin and the host fill (held to their models by the CPU suites) in the order finalize() applies them."""
    g = make_grid(raw)
    out = list(raw)
    if cfg.fill_nodata_radius > 0:
        out = grid_bands(pcr.fill_nodata(g, cfg.fill_nodata_radius, [0, 1]))
    if not cfg.ground.source_band:
        return out
    cell = max(abs(cfg.grid.cell_size_x), abs(cfg.grid.cell_size_y))
    dtm = grid_bands(pcr.ground_filter(g, 0, cfg.ground, cell))[0]
    if cfg.fill_nodata_radius > 0:
        dtm = grid_bands(pcr.fill_nodata(make_grid([dtm]), cfg.fill_nodata_radius))[0]
    out.append(dtm)
    if cfg.ground.top_band:
        out.append(difference(out[1], dtm))
    return out
