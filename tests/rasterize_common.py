"""Shared by tests/test_rasterize.py and tests/test_gpu_rasterize.py: the brute-force model of polygon rasterization (the
contract of csrc/rasterize.hpp) -- no engine code: every cell against every edge, NumPy float64 scalars, which do no FMA -- the
polygon generators, and the ways the tests reach the host twin and the kernels."""
import ctypes as C
import math

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
NAN_BITS = np.uint32(0x7FC00000)
SENTINEL = F32(-12345.5)


def nan32():
    return np.array([NAN_BITS], np.uint32).view(F32)[0]


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} cells differ bitwise, first at {np.argwhere(bad)[:3].tolist()}: "
                           f"{got.view(np.uint32)[bad][:3]} != {want.view(np.uint32)[bad][:3]}")


# ---- polygon sets as plain arrays ------------------------------------------------------------------------------------------------
class Polys:
    """coords (V, 2) float64, ring_offsets (R + 1) int64, polygon_offsets (P + 1) int64, values (P) float32 or None."""

    def __init__(self, polygons, values=None):
        """polygons: a list of polygons, each a list of rings, each an (n, 2) array-like."""
        coords, ro, po = [], [0], [0]
        for rings in polygons:
            for ring in rings:
                ring = np.asarray(ring, F64).reshape(-1, 2)
                coords.append(ring)
                ro.append(ro[-1] + len(ring))
            po.append(len(ro) - 1)
        self.coords = np.ascontiguousarray(np.concatenate(coords) if coords else np.zeros((0, 2)), F64)
        self.ring_offsets = np.array(ro, I64)
        self.polygon_offsets = np.array(po, I64)
        self.values = None if values is None else np.ascontiguousarray(values, F32)

    @property
    def P(self):
        return len(self.polygon_offsets) - 1

    def polygon(self, p):
        """The rings of polygon p, as arrays."""
        return [self.coords[self.ring_offsets[j]:self.ring_offsets[j + 1]]
                for j in range(self.polygon_offsets[p], self.polygon_offsets[p + 1])]

    def subset(self, order):
        vals = None if self.values is None else self.values[list(order)]
        return Polys([self.polygon(p) for p in order], vals)

    def to_pcr(self):
        import pcr
        return pcr.PolygonSet(self.coords, self.ring_offsets, self.polygon_offsets, self.values)


class Geom:
    """The fields of a grid the cell centres are made of; cx, cy: GridConfig::cell_to_world's expression in float64 scalars."""

    def __init__(self, w, h, min_x=0.0, max_y=None, csx=1.0, csy=-1.0):
        self.w, self.h, self.csx, self.csy = int(w), int(h), F64(csx), F64(csy)
        self.min_x = F64(min_x)
        self.max_y = F64(h * abs(csy) if max_y is None else max_y)

    def cx(self, c):
        return self.min_x + (F64(c) + F64(0.5)) * self.csx

    def cy(self, r):
        return self.max_y + (F64(r) + F64(0.5)) * self.csy

    def bounds(self):
        """(min_x, min_y, max_x, max_y) of a BBox whose corner (min_x, max_y) is the origin."""
        x1 = float(self.min_x) + self.w * abs(float(self.csx))
        y0 = float(self.max_y) - self.h * abs(float(self.csy))
        return float(self.min_x), y0, x1, float(self.max_y)

    def cabi(self, A):
        b = self.bounds()
        return A.Grid(b[0], b[1], b[2], b[3], float(self.csx), float(self.csy), self.w, self.h, 4096, 4096, 0, self.h, 0, self.h)

    def config(self):
        import pcr
        g = pcr.GridConfig()
        g.bounds = pcr.BBox(*self.bounds())
        g.cell_size_x, g.cell_size_y = float(self.csx), float(self.csy)
        g.width, g.height = self.w, self.h
        g.tiles_x = (self.w + g.tile_width - 1) // g.tile_width
        g.tiles_y = (self.h + g.tile_height - 1) // g.tile_height
        return g


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model(polys, geom, background=None):
    """Per cell, per polygon, per edge: the edge rule, the parity, the greatest index."""
    bg = nan32() if background is None else F32(background)
    out = np.full((geom.h, geom.w), bg, F32)
    cxs = [geom.cx(c) for c in range(geom.w)]
    with np.errstate(all="ignore"):
        for p in range(polys.P):
            value = F32(p + 1) if polys.values is None else polys.values[p]
            edges = []
            for ring in polys.polygon(p):
                n = len(ring)
                for i in range(n):
                    a, b = ring[i], ring[(i + 1) % n]
                    if a[1] > b[1]:
                        a, b = b, a
                    edges.append((F64(a[0]), F64(a[1]), F64(b[0]), F64(b[1])))
            for r in range(geom.h):
                cy = geom.cy(r)
                xcs = []
                for ax, ay, bx, by in edges:
                    if ay <= cy < by:
                        t = (cy - ay) / (by - ay)
                        xcs.append(ax + t * (bx - ax))
                if not xcs:
                    continue
                xcs = np.array(xcs, F64)
                for c in range(geom.w):
                    if int((xcs > cxs[c]).sum()) % 2 == 1:
                        out[r, c] = value
    return out


# ---- generators ------------------------------------------------------------------------------------------------------------------
def ngon(cx, cy, radius, n, phase=0.1):
    a = phase + 2.0 * math.pi * np.arange(n) / n
    return np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], axis=1)


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], F64)


def comb(x0, y0, teeth=40, pitch=3.0, depth=5.0, spine=1.5):
    """A comb whose `teeth` teeth point up: a row through the teeth has 2 * teeth crossings."""
    pts = [(x0, y0), (x0 + teeth * pitch, y0), (x0 + teeth * pitch, y0 + spine)]
    for i in reversed(range(teeth)):
        xa, xb = x0 + i * pitch, x0 + i * pitch + 0.55 * pitch
        pts += [(xb, y0 + spine), (xb, y0 + spine + depth), (xa, y0 + spine + depth), (xa, y0 + spine)]
    return np.array(pts, F64)


def donut(cx, cy, outer, inner, n=24):
    return [ngon(cx, cy, outer, n), ngon(cx, cy, inner, n, phase=0.3)[::-1]]


def partition(x0, y0, x1, y1, nx, ny, seed, wiggle=3, amp=0.12):
    """The rectangle cut into nx * ny polygons along a jittered lattice; the shared edges are wiggly polylines whose vertices
    BOTH neighbours take from one array, so they share bits.  -> a list of one-ring polygons."""
    rng = np.random.default_rng(seed)
    dx, dy = (x1 - x0) / nx, (y1 - y0) / ny
    node = np.zeros((ny + 1, nx + 1, 2))
    for j in range(ny + 1):
        for i in range(nx + 1):
            jx = 0.0 if i in (0, nx) else rng.uniform(-0.3, 0.3) * dx
            jy = 0.0 if j in (0, ny) else rng.uniform(-0.3, 0.3) * dy
            node[j, i] = (x0 + i * dx + jx, y0 + j * dy + jy)

    def polyline(a, b, straight):
        t = np.linspace(0.0, 1.0, wiggle + 2)[1:-1, None]
        mid = a + t * (b - a)
        if not straight:
            nrm = np.array([-(b - a)[1], (b - a)[0]])
            mid = mid + rng.uniform(-amp, amp, (wiggle, 1)) * nrm
        return np.concatenate([a[None], mid, b[None]])

    hor = [[polyline(node[j, i], node[j, i + 1], j in (0, ny)) for i in range(nx)] for j in range(ny + 1)]
    ver = [[polyline(node[j, i], node[j + 1, i], i in (0, nx)) for i in range(nx + 1)] for j in range(ny)]
    out = []
    for j in range(ny):
        for i in range(nx):
            ring = np.concatenate([hor[j][i][:-1], ver[j][i + 1][:-1], hor[j + 1][i][::-1][:-1], ver[j][i][::-1][:-1]])
            out.append([ring])
    return out


# ---- the host twin and the kernels through the C-ABI ---------------------------------------------------------------------------
def strided(a, stride, offset=0):
    h, w = a.shape
    buf = np.full(offset + h * stride + 7, SENTINEL, F32)
    view = np.lib.stride_tricks.as_strided(buf[offset:], (h, w), (4 * stride, 4))
    view[...] = a
    return buf, view


def sentinels_survive(buf, w, h, stride, offset=0):
    keep = np.ones(buf.shape, bool)
    for r in range(h):
        keep[offset + r * stride: offset + r * stride + w] = False
    assert (buf[keep].view(np.uint32) == np.array([SENTINEL], F32).view(np.uint32)[0]).all(), "a cell outside the band was written"


def _args(A, polys, geom, background):
    g = geom.cabi(A)
    p = A.RasterizeParams() if background is None else A.RasterizeParams(background=background)
    ptr = lambda a: None if a is None else a.ctypes.data
    V, R, P = len(polys.coords), len(polys.ring_offsets) - 1, polys.P
    return g, p, (ptr(polys.coords), V, ptr(polys.ring_offsets), R, ptr(polys.polygon_offsets), P, ptr(polys.values))


def host_cabi(A, polys, geom, background=None, stride=None, offset=0):
    """pcr_hip_rasterize_polygons_host on a strided host band between sentinels."""
    L = A.lib()
    w, h = geom.w, geom.h
    stride = stride or w
    buf, view = strided(np.zeros((h, w), F32), stride, offset)
    g, p, a = _args(A, polys, geom, background)
    A.check(L.pcr_hip_rasterize_polygons_host(C.byref(g), *a, C.byref(p), buf.ctypes.data + 4 * offset, stride))
    sentinels_survive(buf, w, h, stride, offset)
    return view.copy()


def host_cabi_error(A, polys, geom, out=True, stride=None, **over):
    """The return code and message of a call that is expected to be refused; `over` replaces positional arguments by name."""
    L = A.lib()
    w, h = geom.w, geom.h
    buf = np.zeros(h * (stride or w) + 8, F32)
    g, p, a = _args(A, polys, geom, None)
    names = ("coords", "V", "ring_offsets", "R", "polygon_offsets", "P", "values")
    a = [over.get(n, v) for n, v in zip(names, a)]
    rc = L.pcr_hip_rasterize_polygons_host(over.get("grid", C.byref(g)), *a, over.get("params", C.byref(p)),
                                           over.get("out_ptr", buf.ctypes.data if out else None), stride or w)
    return rc, L.pcr_hip_last_error().decode()


def device_cabi(A, polys, geom, background=None, stride=None, offset=0, work_bytes=None):
    """pcr_hip_rasterize_polygons on a strided device band between sentinels."""
    L = A.lib()
    w, h = geom.w, geom.h
    stride = stride or w
    buf, _ = strided(np.zeros((h, w), F32), stride, offset)
    d_out = A.DeviceBuffer.from_numpy(buf)
    g, p, a = _args(A, polys, geom, background)
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_rasterize_work_bytes(a[1], a[5], w, h, C.byref(nbytes)))
    d_work = A.DeviceBuffer(nbytes.value)
    A.check(L.pcr_hip_rasterize_polygons(C.byref(g), *a, C.byref(p), d_out.ptr.value + 4 * offset, stride, d_work.ptr,
                                         nbytes.value if work_bytes is None else work_bytes, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    got = d_out.to_numpy(F32, buf.shape)
    sentinels_survive(got, w, h, stride, offset)
    d_out.free()
    d_work.free()
    return np.lib.stride_tricks.as_strided(got[offset:], (h, w), (4 * stride, 4)).copy()
