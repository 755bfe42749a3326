"""Shared by tests/test_terrain.py and tests/test_gpu_terrain*.py: the NumPy model of the terrain bands (the contract of
csrc/terrain.hpp) -- no engine code: float64 and float32 arrays only, every operation one rounded NumPy operation in the
contract's order, atan_deg restated op for op, the light constants taken from pcr.terrain_light -- and surface generators."""
import numpy as np

import ground_filter_common as G
import overviews_common as M
import pcr

NAN_BITS = M.NAN_BITS
make_grid, grid_bands, values, bits_equal = M.make_grid, M.grid_bands, M.values, G.bits_equal

P = pcr.TerrainProduct
PRODUCTS = [P.SlopeDegrees, P.SlopePercent, P.Aspect, P.Hillshade, P.TRI, P.TPI, P.Roughness]
NAMES = ["slope", "slope_percent", "aspect", "hillshade", "tri", "tpi", "roughness"]
F32, F64 = np.float32, np.float64

TAN_3PI_8, TAN_PI_8 = F32(2.414213562373095), F32(0.4142135623730950)


def spec(**kw):
    s = pcr.TerrainSpec()
    for k, v in kw.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    return s


def atan_deg(x):
    """csrc/terrain.hpp atan_deg on a float32 array of values >= 0 (or NaN): binary32 operations, each rounded."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(all="ignore"):
        big, mid = x > TAN_3PI_8, (x > TAN_PI_8) & ~(x > TAN_3PI_8)
        y = np.where(big, F32(1.5707963267948966), np.where(mid, F32(0.7853981633974483), F32(0.0))).astype(F32)
        t = np.where(big, -(F32(1.0) / x), np.where(mid, (x - F32(1.0)) / (x + F32(1.0)), x)).astype(F32)
        z = t * t
        u = F32(8.05374449538e-2) * z
        u = u - F32(1.38776856032e-1)
        u = u * z
        u = u + F32(1.99777106478e-1)
        u = u * z
        u = u - F32(3.33329491539e-1)
        u = u * z
        u = u * t
        u = u + t
        y = y + u
        out = y * F32(57.29577951308232)
    assert out.dtype == F32
    return out


def window(src, edges):
    """(w9, ok): the nine float32 planes a..i with the missing neighbours dealt with, and the cells that are not NaN by rule."""
    src = np.ascontiguousarray(src, F32)
    h, w = src.shape
    p = np.full((h + 2, w + 2), np.nan, F32)
    p[1:h + 1, 1:w + 1] = src
    w9 = [p[dr:dr + h, dc:dc + w].copy() for dr in range(3) for dc in range(3)]
    e = w9[4]
    ok = ~np.isnan(e)
    for k in range(9):
        if k == 4:
            continue
        miss = np.isnan(w9[k])
        if edges:
            w9[k] = np.where(miss, e, w9[k])
        else:
            ok &= ~miss
    return w9, ok


def terrain(src, products, z_factor=1.0, edges=False, azimuth=315.0, altitude=45.0, cell_size_x=1.0, cell_size_y=-1.0):
    """[len(products), h, w] float32: the contract, product by product."""
    w9, ok = window(src, edges)
    with np.errstate(all="ignore"):                                   # (a signalling NaN is converted)
        a, b, c, d, e, f, g, h, i = [x.astype(F64) for x in w9]
    z = float(F32(z_factor))
    kx, ky = F64(z) / (F64(8.0) * F64(cell_size_x)), F64(z) / (F64(-8.0) * F64(cell_size_y))
    sin_alt, ls, lc = (F64(v) for v in pcr.terrain_light(float(F32(azimuth)), float(F32(altitude))))
    out = []
    with np.errstate(all="ignore"):
        gx = ((c + 2.0 * f) + i) - ((a + 2.0 * d) + g)
        gy = ((a + 2.0 * b) + c) - ((g + 2.0 * h) + i)
        p, q = gx * kx, gy * ky
        s2 = p * p + q * q
        for prod in products:
            if prod == P.SlopeDegrees:
                r = atan_deg(np.sqrt(s2).astype(F32))
            elif prod == P.SlopePercent:
                r = (100.0 * np.sqrt(s2)).astype(F32)
            elif prod == P.Aspect:
                t = atan_deg((np.abs(p) / np.abs(q)).astype(F32))
                north = np.where(p > 0.0, F32(360.0) - t, t)
                south = np.where(p > 0.0, F32(180.0) + t, F32(180.0) - t)
                r = np.where(q <= 0.0, north, south).astype(F32)
                r = np.where(r == F32(360.0), F32(0.0), r)
                r = np.where((p == 0.0) & (q == 0.0), F32(-1.0), r).astype(F32)
            elif prod == P.Hillshade:
                L = (sin_alt - (p * ls + q * lc)) / np.sqrt(1.0 + s2)
                r = np.where(L <= 0.0, F32(1.0), (1.0 + 254.0 * L).astype(F32)).astype(F32)
            elif prod == P.TRI:
                s = np.abs(a - e) + np.abs(b - e)
                for v in (c, d, f, g, h, i):
                    s = s + np.abs(v - e)
                r = (s / 8.0).astype(F32)
            elif prod == P.TPI:
                s = a + b
                for v in (c, d, f, g, h, i):
                    s = s + v
                r = (e - s / 8.0).astype(F32)
            elif prod == P.Roughness:
                hi, lo = w9[0].copy(), w9[0].copy()
                for v in w9[1:]:
                    hi = np.where(v > hi, v, hi)
                    lo = np.where(v < lo, v, lo)
                r = hi - lo
                assert r.dtype == F32
            else:
                raise AssertionError(prod)
            r = np.ascontiguousarray(r, F32).copy()
            r.view(np.uint32)[np.isnan(r) | ~ok] = NAN_BITS
            out.append(r)
    return np.stack(out)


def host(src, products, sp=None, cell_size_x=1.0, cell_size_y=-1.0, threads=0):
    from pcr import _pcr
    return np.array(_pcr._terrain_host(np.ascontiguousarray(src, F32), list(products), sp, cell_size_x, cell_size_y, threads))


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def plane(w, h, alpha, beta, cell_size_x=1.0, cell_size_y=-1.0, z0=100.0):
    """z = alpha * x + beta * y at the cell centres: x grows with the column by cell_size_x, y with the row by cell_size_y."""
    rr, cc = np.mgrid[0:h, 0:w]
    return (z0 + alpha * (cc * cell_size_x) + beta * (rr * cell_size_y)).astype(F32)


def hills(w, h, seed, nan_fraction=0.0):
    """A rolling surface with some noise, metres on a 1 m grid: slopes of a few tens of degrees in every direction."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:h, 0:w]
    z = 50.0 + 8.0 * np.sin(cc / 7.0) * np.cos(rr / 5.0) + 0.3 * cc - 0.2 * rr + rng.normal(0.0, 0.05, (h, w))
    z = z.astype(F32)
    z[rng.random((h, w)) < nan_fraction] = np.nan
    return z


def ramp(w, h, lo=-20.0, hi=20.0):
    """A band whose interior cells have s2 spread densely over 2^(2 lo) .. 2^(2 hi): column c is a plane in x of gradient
    2^e(c) per cell (GY = 0), with a per-row wobble of the gradient's last bits so that the arguments of sqrt and / differ
    from row to row."""
    out = np.zeros((h, w), F64)
    ex = np.linspace(lo, hi, w // 3)
    rng = np.random.default_rng(99)
    for k, e in enumerate(ex):
        for r in range(h):
            g = 2.0 ** e * (1.0 + rng.random())
            base = rng.normal(0.0, 1.0) * g * 4
            out[r, 3 * k:3 * k + 3] = [base - g, base, base + g]
    return out[:, :3 * len(ex)].astype(F32)


# ---- the pipelines' common ground --------------------------------------------------------------------------------------------
def band_cfg(source, product, name="", **kw):
    t = pcr.TerrainBandConfig()
    t.source_band, t.product, t.band_name = source, product, name
    for k, v in kw.items():
        assert hasattr(t, k), k
        setattr(t, k, v)
    return t


def expect_bands(sources, cfg):
    """The terrain bands of cfg.terrain in list order, from the result's other bands by name (as they leave the pipeline):
    the host loop, which the CPU suite holds to the model."""
    out = []
    for t in cfg.terrain:
        sp = spec(z_factor=t.z_factor, compute_edges=t.compute_edges, azimuth=t.azimuth, altitude=t.altitude)
        out.append(host(sources[t.source_band], [t.product], sp, cfg.grid.cell_size_x, cfg.grid.cell_size_y)[0])
    return out
