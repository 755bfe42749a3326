"""Shared by tests/test_fill_nodata.py and tests/test_gpu_fill_nodata.py: the NumPy model of fill_nodata (the contract of
csrc/fill_nodata.hpp), the value mix (overviews_common.values) and the hole masks the fills are checked on."""
import numpy as np

import overviews_common as M
import pcr

NAN_BITS = M.NAN_BITS
bits_equal, make_grid, grid_bands, values = M.bits_equal, M.make_grid, M.grid_bands, M.values


def fill(src, R):
    """fill(src, R): binary64 sums over the disc in row-major window order, w = 1.0f / (float)d2, never chained."""
    src = np.ascontiguousarray(src, np.float32)
    h, w = src.shape
    p = np.full((h + 2 * R, w + 2 * R), np.nan, np.float32)
    p[R:R + h, R:R + w] = src
    s = np.zeros((h, w), np.float64)
    t = np.zeros((h, w), np.float64)
    with np.errstate(all="ignore"):
        for dr in range(-R, R + 1):
            for dc in range(-R, R + 1):
                d2 = dr * dr + dc * dc
                if d2 == 0 or d2 > R * R:
                    continue
                wgt = np.float32(1.0) / np.float32(d2)
                v = p[R + dr:R + dr + h, R + dc:R + dc + w]
                ok = ~np.isnan(v)
                s += np.where(ok, np.float64(wgt) * v.astype(np.float64), 0.0)       # adding +0.0 equals skipping
                t += np.where(ok, np.float64(wgt), 0.0)
        out = src.copy()
        hit = np.isnan(src) & (t > 0)
        f = (s[hit] / t[hit]).astype(np.float32)
    f.view(np.uint32)[np.isnan(f)] = NAN_BITS              # Inf + -Inf among the neighbours: one NaN on every machine
    out[hit] = f
    return out


NAN_PAYLOADS = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001], np.uint32)


def punch(a, mask, seed=0):
    """`a` with NaNs of several payloads where `mask` is set."""
    out = a.copy()
    rng = np.random.default_rng(seed)
    out.view(np.uint32)[mask] = rng.choice(NAN_PAYLOADS, int(mask.sum()))
    return out


def isolated(w, h, fraction, seed):
    return np.random.default_rng(seed).uniform(size=(h, w)) < fraction


def blobs(w, h, count, radius, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(count):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.uniform(1.0, radius)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m


def full_rows(w, h, rows):
    m = np.zeros((h, w), bool)
    m[list(rows), :] = True
    return m


def finite_values(w, h, seed):
    """Plain finite values without a NaN: what a hole mask is punched into when the NaN cells must be exactly the mask."""
    return np.random.default_rng(seed).normal(100.0, 30.0, (h, w)).astype(np.float32)


# ---- the pipelines' common ground ----------------------------------------------------------------------------------------------
def pipeline_cfg(W, H, mode, radius=0):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    assert (cfg.grid.width, cfg.grid.height) == (W, H)
    cfg.exec_mode = mode
    specs = []
    for t in (pcr.ReductionType.Average, pcr.ReductionType.Count, pcr.ReductionType.Max):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", t
        specs.append(r)
    cfg.reductions = specs
    cfg.fill_nodata_radius = radius
    return cfg


FILLED_BANDS = (0, 2)          # Average and Max of pipeline_cfg; Count (1) stays as it is


def cloud(W, H, n, seed):
    rng = np.random.default_rng(seed)
    c = pcr.PointCloud.create(n)
    c.set_x_array(rng.uniform(0.0, W * 0.9, n))                # the right tenth stays empty: a void wider than any radius used
    c.set_y_array(rng.uniform(0.0, H, n))
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", rng.normal(0.0, 100.0, n).astype(np.float32))
    return c


def expect_filled(raw_bands, radius):
    """What a pipeline with fill_nodata_radius = radius returns, from the bands of the same pipeline with radius 0."""
    return [fill(b, radius) if i in FILLED_BANDS else b for i, b in enumerate(raw_bands)]
