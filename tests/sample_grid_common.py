"""Shared by tests/test_sample_grid.py and tests/test_gpu_sample_grid.py: the NumPy model of sampling a band at points (the
contract of csrc/sample_grid.hpp) -- no engine code: float64 arithmetic, every operation one rounded NumPy operation in the
contract's order, one astype(float32) -- and the builders of surfaces, lattices and clouds."""
import ctypes as C

import numpy as np

F32, F64 = np.float32, np.float64
NAN_BITS = 0x7FC00000
NEAREST, BILINEAR = 0, 1

# (width, height) of the surfaces every comparison runs over
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (33, 65)]


class Surface:
    """One Float32 band with a geometry of its own."""

    def __init__(self, band, min_x, max_y, csx, csy):
        self.band = np.ascontiguousarray(band, F32)
        self.h, self.w = self.band.shape
        self.csx, self.csy = float(csx), float(csy)
        # bounds as a GridConfig has them, whatever the signs; the origin stays (min_x, max_y), so on a south-up surface
        # (cell_size_y > 0) every quotient is <= 0 and the rows clamp to 0, exactly as the routing answers for such a grid
        self.min_x, self.max_x = float(min_x), float(min_x + self.w * abs(self.csx))
        self.max_y, self.min_y = float(max_y), float(max_y - self.h * abs(self.csy))

    def bounds(self):
        return (self.min_x, self.min_y, self.max_x, self.max_y)


def canonical(a):
    """float32 array with every NaN made 0x7FC00000."""
    a = np.ascontiguousarray(a, F32).copy()
    a.view(np.uint32)[np.isnan(a)] = NAN_BITS
    return a


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def bits_equal(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} differ, first at {bad[:5].tolist()}: got "
                           f"{[hex(v) for v in g.ravel()[bad[:5]]]} want {[hex(v) for v in w.ravel()[bad[:5]]]}")


def model(s, x, y, z=None, mode=BILINEAR):
    """The contract, restated: float64 operations one at a time, one rounding to float32 at the end."""
    x, y = np.ascontiguousarray(x, F64), np.ascontiguousarray(y, F64)
    n = x.size
    with np.errstate(all="ignore"):
        inside = (x >= s.min_x) & (x <= s.max_x) & (y >= s.min_y) & (y <= s.max_y)
        xs, ys = np.where(inside, x, s.min_x), np.where(inside, y, s.max_y)
        qx = (xs - F64(s.min_x)) / F64(s.csx)
        qy = (ys - F64(s.max_y)) / F64(s.csy)
        col = np.clip(np.floor(qx), 0, s.w - 1).astype(np.int64)
        row = np.clip(np.floor(qy), 0, s.h - 1).astype(np.int64)
        e = s.band[row, col]
        if mode == NEAREST:
            smp = e.astype(F64)
            direct = e
        else:
            tx = (qx - col.astype(F64)) - F64(0.5)
            ty = (qy - row.astype(F64)) - F64(0.5)
            ncol = np.where(tx < 0, col - 1, col + 1)
            nrow = np.where(ty < 0, row - 1, row + 1)
            wx, wy = np.where(tx < 0, -tx, tx), np.where(ty < 0, -ty, ty)
            h_in, v_in = (ncol >= 0) & (ncol < s.w), (nrow >= 0) & (nrow < s.h)
            cc, rr = np.where(h_in, ncol, col), np.where(v_in, nrow, row)
            h, v, d = s.band[row, cc], s.band[rr, col], s.band[rr, cc]
            h = np.where(np.isnan(h), e, h)                  # (a column or row outside the band is e's own: cc, rr)
            v = np.where(np.isnan(v), e, v)
            d = np.where(np.isnan(d), e, d)
            ux, uy = F64(1.0) - wx, F64(1.0) - wy
            smp = (ux * uy) * e.astype(F64)
            smp = smp + (wx * uy) * h.astype(F64)
            smp = smp + (ux * wy) * v.astype(F64)
            smp = smp + (wx * wy) * d.astype(F64)
            direct = None
        if z is not None:
            out = (np.ascontiguousarray(z, F32).astype(F64) - smp).astype(F32)
        elif direct is not None:
            out = direct.copy()                      # Nearest: the cell's bits
        else:
            out = smp.astype(F32)
    out = np.where(inside, out, F32(np.nan)).astype(F32)
    assert out.shape == (n,)
    return canonical(out)


# ---- surfaces -------------------------------------------------------------------------------------------------------------
def make_surface(w, h, seed, csx=1.5, csy=-0.75, min_x=1000.25, max_y=5000.5, nan_frac=0.2, infs=True):
    rng = np.random.default_rng(seed)
    band = (rng.standard_normal((h, w)) * 30.0 + 100.0).astype(F32)
    if nan_frac > 0:
        band[rng.random((h, w)) < nan_frac] = np.nan
    if infs and w * h >= 4:
        flat = band.ravel()
        at = rng.choice(w * h, 2, replace=False)
        flat[at[0]], flat[at[1]] = np.inf, -np.inf
    if w * h > 16:
        band.ravel()[rng.integers(0, w * h)] = F32(1e-42)            # a denormal
    return Surface(band, min_x, max_y, csx, csy)


def surfaces(seed=7):
    """The five shapes, north-up and south-up, cell_size_x != |cell_size_y|, a 20 % NaN sprinkle, +-Inf cells."""
    out = []
    for k, (w, h) in enumerate(SHAPES):
        out.append((f"{w}x{h}-north", make_surface(w, h, seed + k)))
        out.append((f"{w}x{h}-south", make_surface(w, h, seed + 50 + k, csx=0.5, csy=2.0, min_x=-37.5, max_y=12.0)))
    return out


def lattice(s, rng=None, random_points=600):
    """Cell centres, cell edges, corners, every outer edge and corner of the bounds, one ulp either side of each, points
    outside, NaN coordinates -- plus random points over (and a little beyond) the bounds."""
    def axis(origin, cs, n, lo, hi):
        v = []
        for k in range(n + 1):
            edge = origin + k * cs
            v += [edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf)]
            if k < n:
                c = origin + (k + 0.5) * cs
                v += [c, np.nextafter(c, -np.inf), np.nextafter(c, np.inf), origin + (k + 0.25) * cs, origin + (k + 0.8125) * cs]
        v += [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
              lo - 3.0 * abs(cs), hi + 3.0 * abs(cs), np.nan]
        return np.array(v, F64)
    # (a large surface's lattice is thinned: the values around its first and last cells are kept whole, every few in between)
    ax = axis(s.min_x, s.csx, s.w, s.min_x, s.max_x)
    ay = axis(s.max_y, s.csy, s.h, s.min_y, s.max_y)
    if ax.size * ay.size > 60000:
        keep_x = np.r_[0:24, ax.size - 33:ax.size, np.arange(24, ax.size - 33, 5)]
        keep_y = np.r_[0:24, ay.size - 33:ay.size, np.arange(24, ay.size - 33, 7)]
        ax, ay = ax[np.unique(keep_x)], ay[np.unique(keep_y)]
    gx, gy = np.meshgrid(ax, ay)
    x, y = gx.ravel(), gy.ravel()
    if rng is not None and random_points:
        mx, my = 0.1 * (s.max_x - s.min_x), 0.1 * (s.max_y - s.min_y)
        x = np.r_[x, rng.uniform(s.min_x - mx, s.max_x + mx, random_points)]
        y = np.r_[y, rng.uniform(s.min_y - my, s.max_y + my, random_points)]
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def values_for(n, rng):
    """A value channel: ordinary heights, with NaN, +-Inf and a denormal among them."""
    z = (rng.standard_normal(n) * 40.0 + 120.0).astype(F32)
    if n >= 8:
        z[rng.integers(0, n, max(n // 50, 1))] = np.nan
        z[rng.integers(0, n)] = np.inf
        z[rng.integers(0, n)] = -np.inf
        z[rng.integers(0, n)] = F32(1e-42)
    return z


# ---- the C-ABI's host loop -------------------------------------------------------------------------------------------------
def cabi_grid(A, s):
    return A.make_grid(s.bounds(), cell=(s.csx, s.csy), dims=(s.w, s.h), tile=(max(s.w, 1), max(s.h, 1)))


def host_loop(A, s, x, y, z=None, mode=BILINEAR, out=None, band=None, stride=None):
    """pcr_hip_sample_grid_host over NumPy arrays; `out` may be z itself (in place)."""
    L = A.lib()
    x, y = np.ascontiguousarray(x, F64), np.ascontiguousarray(y, F64)
    band = s.band if band is None else band
    stride = s.w if stride is None else stride
    if out is None:
        out = np.full(x.size, 123.0, F32)
    g = cabi_grid(A, s)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.pcr_hip_sample_grid_host(C.byref(g), ptr(band), stride, ptr(x), ptr(y), ptr(z), x.size, mode, ptr(out))
    assert rc == 0, L.pcr_hip_last_error()
    return out


# ---- the package's containers ----------------------------------------------------------------------------------------------
def pcr_grid(pcr, s, location=None, crs=None, extra_bands=0):
    """A pcr.Grid that holds the surface in its LAST band (bands before it are decoys), tagged with the surface's geometry."""
    descs = []
    for k in range(extra_bands + 1):
        d = pcr.BandDesc()
        d.name = f"b{k}"
        descs.append(d)
    g = pcr.Grid.create(s.w, s.h, descs)
    for k in range(extra_bands):
        g.set_band_array(k, np.full((s.h, s.w), -7.0, F32))
    g.set_band_array(extra_bands, s.band)
    g.set_geometry(grid_config(pcr, s, crs))
    return g if location is None else g.to(location)


def grid_config(pcr, s, crs=None):
    gc = pcr.GridConfig()
    b = pcr.BBox()
    b.min_x, b.min_y, b.max_x, b.max_y = s.bounds()
    gc.bounds = b
    gc.cell_size_x, gc.cell_size_y = s.csx, s.csy
    gc.width, gc.height = s.w, s.h
    gc.tile_width, gc.tile_height = max(s.w, 1), max(s.h, 1)
    gc.tiles_x = gc.tiles_y = 1
    if crs is not None:
        gc.crs = crs
    return gc


def make_cloud(pcr, x, y, channels, location=None, crs=None):
    """location: None (Host), pcr.MemoryLocation.HostPinned or .Device."""
    n = len(x)
    pinned = location == pcr.MemoryLocation.HostPinned
    c = pcr.PointCloud.create(max(n, 1), pcr.MemoryLocation.HostPinned if pinned else pcr.MemoryLocation.Host)
    c.set_x_array(np.ascontiguousarray(x, F64))
    c.set_y_array(np.ascontiguousarray(y, F64))
    for name, v in channels.items():
        c.add_channel(name, pcr.DataType.Float32)
        c.set_channel_array_f32(name, np.ascontiguousarray(v, F32))
    if crs is not None:
        c.set_crs(crs)
    return c.to_device() if location == pcr.MemoryLocation.Device else c


# ---- pipelines: "derived at ingest == precomputed channel", on either engine -----------------------------------------------
# Every float32 sum below is exact in any order, so that every comparison is view(uint32) equality on the HIP engine too, whose
# atomics fold in no fixed order: point coordinates are multiples of 1/8, the surfaces' origins and cell sizes dyadic, their
# values small integers, z multiples of 1/8 -- a Bilinear sample is then a multiple of 2^-10 below 2^6, z - sample a multiple of
# 2^-10 below 2^7, and a cell's sum of fewer than 2^6 of them fits float32's 24 bits.
PGRID = dict(min_x=0.0, min_y=0.0, max_x=40.0, max_y=24.0, cs=1.0, W=40, H=24, tw=16, th=16)


def dyadic_surface(seed, coarse=False, positive=False):
    """A surface over [2, 38] x [2, 22] of the pipeline grid (points beyond it sample NaN), cells of 0.5 (coarse: 4 x 2, coarser
    than the grid's), integer values, a 10 % NaN sprinkle."""
    rng = np.random.default_rng(seed)
    csx, csy = (4.0, -2.0) if coarse else (0.5, -0.5)
    w, h = int(36 / csx), int(20 / -csy)
    band = rng.integers(1 if positive else -32, 5 if positive else 33, (h, w)).astype(F32)
    band[rng.random((h, w)) < 0.1] = np.nan
    return Surface(band, 2.0, 22.0, csx, csy)


def dyadic_points(n, seed, g=PGRID):
    """x, y multiples of 1/8 over (and a little beyond) the grid; z multiples of 1/8 in [0, 64); cls 1 / 2 / 5; ret 1..3; t small
    integers; dir a multiple of pi / 8."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 8 * int(g["max_x"]) + 9, n) / 8.0
    y = rng.integers(-8, 8 * int(g["max_y"]) + 9, n) / 8.0
    return dict(x=x, y=y, z=(rng.integers(0, 512, n) / 8.0).astype(F32), cls=rng.choice(np.array([1, 2, 5], F32), n),
                ret=rng.integers(1, 4, n).astype(F32), t=rng.integers(0, 6, n).astype(F32),
                dir=(rng.integers(0, 8, n) * (np.pi / 8.0)).astype(F32))


def one_point_per_cell(seed, g=PGRID):
    """One point somewhere inside every cell (any coordinates: nothing is summed), z any float."""
    rng = np.random.default_rng(seed)
    col, row = np.meshgrid(np.arange(g["W"]), np.arange(g["H"]))
    x = g["min_x"] + (col.ravel() + rng.uniform(0.05, 0.95, col.size)) * g["cs"]
    y = g["max_y"] - (row.ravel() + rng.uniform(0.05, 0.95, col.size)) * g["cs"]
    return dict(x=x, y=y, z=(rng.standard_normal(col.size) * 20.0 + 50.0).astype(F32))


def channel_configs(pcr, chans):
    """chans: [(name, value_channel or "", NEAREST | BILINEAR)] -> [pcr.SurfaceChannelConfig]"""
    modes = {NEAREST: pcr.SampleMode.Nearest, BILINEAR: pcr.SampleMode.Bilinear}
    return [pcr.SurfaceChannelConfig(name, value, modes[mode]) for name, value, mode in chans]


def with_model_channels(c, chans, surfs, x=None, y=None):
    """The cloud dict with every surface channel added as the model computes it (at x, y when given: the reprojected ones)."""
    out = dict(c)
    px, py = (c["x"], c["y"]) if x is None else (x, y)
    for name, value, mode in chans:
        out[name] = model(surfs[name], px, py, c[value] if value else None, mode)
    return out


def dict_cloud(pcr, c, location=None, crs=None):
    return make_cloud(pcr, c["x"], c["y"], {k: v for k, v in c.items() if k not in ("x", "y")}, location, crs)


def set_surfaces(pcr, p, surfs, location=None):
    for name, s in surfs.items():
        p.set_surface(name, pcr_grid(pcr, s, location, extra_bands=1), 1)          # (band 1: band 0 is a decoy)


def grid_bands(p):
    res = p.result()
    res = res.to_host() if res.location() != type(res.location()).Host else res
    return [np.array(res.band_array(b)) for b in range(res.num_bands())]


def assert_same_pipelines(p, q, what, collections=True):
    """collections=False: p ingested in chunks what q ingested at once."""
    got, want = grid_bands(p), grid_bands(q)
    assert len(got) == len(want)
    for b, (u, w) in enumerate(zip(got, want)):
        bits_equal(u, w, f"{what}: band {b}")
    a, b = p.stats(), q.stats()
    assert a.points_processed == b.points_processed, what
    assert not collections or a.collections_processed == b.collections_processed, what
    return got


def check_pair(pcr, make_config, specs, chans, ingests, cfg_filt=(), location=None, what="", ingest="ingest", **kw):
    """ingests: [(cloud dict, {surface channel: Surface})].  A pipeline with surface_channels fed the clouds as they are against
    the same pipeline without them fed clouds that already carry the model's channels; set_surface is called before every
    ingest.  Returns the bands."""
    p = pcr.Pipeline.create(make_config(specs, cfg_filt, surface_channels=channel_configs(pcr, chans), **kw))
    assert p is not None, pcr.pipeline_create_error()
    q = pcr.Pipeline.create(make_config(specs, cfg_filt, **kw))
    assert q is not None, pcr.pipeline_create_error()
    alive = []                                                   # (ingest_async: the clouds stay untouched until synchronize())
    for c, surfs in ingests:
        set_surfaces(pcr, p, surfs)
        alive += [dict_cloud(pcr, c, location), dict_cloud(pcr, with_model_channels(c, chans, surfs), location)]
        getattr(p, ingest)(alive[-2])
        getattr(q, ingest)(alive[-1])
    if ingest != "ingest":
        p.synchronize()
        q.synchronize()
    p.finalize()
    q.finalize()
    return assert_same_pipelines(p, q, what)
