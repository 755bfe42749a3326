"""Shared by tests/test_polygonize.py and tests/test_gpu_polygonize.py: the brute-force model of polygonize (the contract of
csrc/polygonize.hpp) -- no engine code: a dict of every boundary edge, the successor as the contract words it, the rings walked
from the sorted corner slots -- the band generators, the structure checks, and the ways the tests reach the host twin and the
kernels."""
import ctypes as C

import numpy as np

import rasterize_common as R

F32, F64, I32, I64, U32 = np.float32, np.float64, np.int32, np.int64, np.uint32
SENTINEL = R.SENTINEL
STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))                    # direction s: top runs +column, right +row, bottom -column, left -row

# (min_x, max_y, csx, csy) by (w, h): the geometries every round trip runs on
GEOMETRIES = (lambda w, h: (0.0, float(h), 1.0, -1.0), lambda w, h: (500000.0, 4500000.0, 0.5, -0.5),
              lambda w, h: (-3.25, 80.7, 1.3, -1.1), lambda w, h: (0.7 * w, 0.05, -0.7, 0.9))


def geom(w, h, k=0):
    min_x, max_y, csx, csy = GEOMETRIES[k](w, h)
    return R.Geom(w, h, min_x=min_x, max_y=max_y, csx=csx, csy=csy)


def zones_of(band):
    """zonal's rule: a whole number in [1, 2^24], else 0."""
    v = np.asarray(band, F32)
    with np.errstate(invalid="ignore"):
        ok = (v >= 1) & (v <= 16777216) & (v == np.floor(v))
    return np.where(ok, v, F32(0)).astype(U32)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model(band):
    """-> the ring table: dict(E, ring_zone uint32 [R], ring_offset int64 [R + 1], vertex_row, vertex_col int32 [V])."""
    z = zones_of(band)
    h, w = z.shape

    def at(r, c):
        return int(z[r, c]) if 0 <= r < h and 0 <= c < w else 0

    succ = {}
    for r in range(h):
        for c in range(w):
            zz = at(r, c)
            if zz == 0:
                continue
            for s in range(4):
                (fr, fc), (orr, oc) = STEP[s], STEP[(s + 3) % 4]
                if at(r + orr, c + oc) == zz:
                    continue                                         # no boundary edge: the cell across has the same zone
                ahead, diag = at(r + fr, c + fc), at(r + fr + orr, c + fc + oc)
                if ahead != zz:
                    succ[(r, c, s)] = (r, c, (s + 1) % 4)
                elif diag == zz:
                    succ[(r, c, s)] = (r + fr + orr, c + fc + oc, (s + 3) % 4)
                else:
                    succ[(r, c, s)] = (r + fr, c + fc, s)
    pred = {}
    for e, n in succ.items():
        assert n in succ and at(n[0], n[1]) == at(e[0], e[1]), f"the successor of {e} is no boundary edge of its zone"
        assert n not in pred, f"{n} has two predecessors"
        pred[n] = e
    assert len(pred) == len(succ)
    slot = lambda e: 4 * (e[0] * w + e[1]) + e[2]
    corners = sorted((e for e in succ if pred[e][2] != e[2]), key=slot)
    seen, ring_zone, ring_offset, vr, vc = set(), [], [0], [], []
    for start in corners:
        if start in seen:
            continue
        e = start
        while True:
            seen.add(e)
            if pred[e][2] != e[2]:
                r, c, s = e
                vr.append(r + (1 if s >= 2 else 0))
                vc.append(c + (1 if s in (1, 2) else 0))
            e = succ[e]
            if e == start:
                break
        ring_zone.append(at(start[0], start[1]))
        ring_offset.append(len(vr))
    return dict(E=len(succ), ring_zone=np.array(ring_zone, U32), ring_offset=np.array(ring_offset, I64),
                vertex_row=np.array(vr, I32), vertex_col=np.array(vc, I32))


def same_table(got, want, what=""):
    assert got["E"] == want["E"], f"{what}: E {got['E']} != {want['E']}"
    for k in ("ring_zone", "ring_offset", "vertex_row", "vertex_col"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), \
            f"{what}: {k} differs ({got[k].shape} against {want[k].shape})"


def set_of(table, g):
    """The table as a polygon set, the host layer's one pass restated: rings grouped by zone (stable), the corners placed by one
    rounded product and one rounded sum (NumPy float64 arrays do no FMA).  -> R.Polys with values."""
    order = np.argsort(table["ring_zone"], kind="stable")
    zones = sorted(set(table["ring_zone"].tolist()))
    x = g.min_x + table["vertex_col"].astype(F64) * g.csx
    y = g.max_y + table["vertex_row"].astype(F64) * g.csy
    xy = np.stack([x, y], axis=1)
    polygons = {zz: [] for zz in zones}
    for j in order:
        polygons[int(table["ring_zone"][j])].append(xy[table["ring_offset"][j]:table["ring_offset"][j + 1]])
    return R.Polys([polygons[zz] for zz in zones], values=[float(zz) for zz in zones])


def as_polys(s):
    """A pcr.PolygonSet as R.Polys."""
    p = R.Polys([])
    p.coords, p.ring_offsets, p.polygon_offsets = np.array(s.coords, F64).reshape(-1, 2), np.array(s.ring_offsets, I64), np.array(s.polygon_offsets, I64)
    p.values = None if s.values is None else np.array(s.values, F32)
    return p


def bits_equal(got, want, what=""):
    """Two polygon sets (pcr.PolygonSet or R.Polys): the coordinates by their bits, offsets and values exactly."""
    got = got if isinstance(got, R.Polys) else as_polys(got)
    want = want if isinstance(want, R.Polys) else as_polys(want)
    for k in ("ring_offsets", "polygon_offsets"):
        assert getattr(got, k).tolist() == getattr(want, k).tolist(), f"{what}: {k} differ"
    assert (got.values is None) == (want.values is None), f"{what}: values"
    if want.values is not None:
        assert (got.values.view(U32) == want.values.view(U32)).all(), f"{what}: values differ"
    a, b = np.ascontiguousarray(got.coords, F64).view(np.uint64), np.ascontiguousarray(want.coords, F64).view(np.uint64)
    assert a.shape == b.shape and (a == b).all(), f"{what}: coordinates differ bitwise"


# ---- what every table must satisfy -------------------------------------------------------------------------------------------------
def check_structure(table, band, what=""):
    """Every ring has at least 4 vertices and no three in a row collinear; per zone the absolute sum of the rings' shoelace sums in
    lattice units (a hole runs the other way round: negative) is the zone's cell count."""
    z = zones_of(band)
    cells = {int(k): int(n) for k, n in zip(*np.unique(z[z > 0], return_counts=True))}
    area = {}
    for j, zz in enumerate(table["ring_zone"].tolist()):
        a, b = table["ring_offset"][j], table["ring_offset"][j + 1]
        r, c = table["vertex_row"][a:b].astype(I64), table["vertex_col"][a:b].astype(I64)
        assert b - a >= 4, f"{what}: ring {j} has {b - a} vertices"
        dr, dc = np.roll(r, -1) - r, np.roll(c, -1) - c
        assert ((dr == 0) != (dc == 0)).all(), f"{what}: ring {j} has an edge that is not along the lattice"
        cross = dr * np.roll(dc, -1) - dc * np.roll(dr, -1)
        assert (cross != 0).all(), f"{what}: ring {j} has three collinear vertices in a row"
        area[zz] = area.get(zz, 0) + int(np.sum(c * np.roll(r, -1) - np.roll(c, -1) * r))
    assert sorted(area) == sorted(cells), f"{what}: zones {sorted(area)[:5]} against {sorted(cells)[:5]}"
    for zz in cells:
        assert abs(area[zz]) == 2 * cells[zz], f"{what}: zone {zz} encloses {abs(area[zz]) / 2} cells of {cells[zz]}"


def burn_target(band):
    """What burning the polygons back must give: the band, its cells of no zone NaN."""
    z = zones_of(band)
    out = z.astype(F32)
    out[z == 0] = R.nan32()
    return out


def centres_strictly_inside(g):
    """The round trip's precondition: every cell centre rounds strictly between its corners' coordinates."""
    j, i = np.arange(g.w + 1, dtype=F64), np.arange(g.h + 1, dtype=F64)
    x, y = g.min_x + j * g.csx, g.max_y + i * g.csy
    cx = g.min_x + (np.arange(g.w, dtype=F64) + 0.5) * g.csx
    cy = g.max_y + (np.arange(g.h, dtype=F64) + 0.5) * g.csy
    assert (np.minimum(x[:-1], x[1:]) < cx).all() and (cx < np.maximum(x[:-1], x[1:])).all()
    assert (np.minimum(y[:-1], y[1:]) < cy).all() and (cy < np.maximum(y[:-1], y[1:])).all()


# ---- generators ------------------------------------------------------------------------------------------------------------------
def blobs(h, w, seed, zones=7, nothing=0.25):
    """Random zones in patches of one to a few cells, a quarter of the cells no zone: saddles, holes, islands, corner touches."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, zones + 1, ((h + 2) // 3 + 1, (w + 2) // 3 + 1))
    a = np.kron(coarse, np.ones((3, 3), int))[:h, :w].astype(F32)
    flip = rng.random((h, w)) < 0.2
    a[flip] = rng.integers(1, zones + 1, int(flip.sum()))
    a[rng.random((h, w)) < nothing] = np.nan
    return a


def checkerboard(h, w, two=True):
    """Zones on the black squares over a background of no zone: every lattice corner a saddle."""
    rr, cc = np.mgrid[0:h, 0:w]
    a = np.full((h, w), np.nan, F32)
    black = (rr + cc) % 2 == 0
    a[black] = (1 + (rr[black] // 2 + cc[black]) % 2) if two else 1
    return a


def serpentine(n=65):
    """One 1-cell-wide path that fills every other row of an n x n band and joins them at alternating ends: one ring."""
    a = np.full((n, n), np.nan, F32)
    a[0::2, :] = 5
    for k, r in enumerate(range(1, n, 2)):
        a[r, n - 1 if k % 2 == 0 else 0] = 5
    return a


def nested():
    """Zone 1 around zone 2 around an island of zone 1 with a background hole beside it; two squares of zone 3 touching at a
    corner, and zone 1 touching itself at a corner."""
    a = np.full((16, 20), np.nan, F32)
    a[1:13, 1:13] = 1
    a[3:11, 3:11] = 2
    a[5:9, 5:8] = 1
    a[6, 6] = np.nan                                                 # a hole in the island
    a[5:9, 8] = np.nan                                               # a background hole in zone 2, beside the island
    a[11, 1] = np.nan
    a[13, 13] = 1                                                    # touches the big square at a corner
    a[2:4, 15:17] = 3
    a[4:6, 17:19] = 3
    return a


def values_band():
    """Every kind of value that is no zone, around the two that are."""
    nan2 = np.array([0x7FC12345, 0xFFC00001], U32).view(F32)
    a = np.array([[1, nan2[0], np.inf, 0, -3, 2.5, 16777216, 16777218],
                  [1, nan2[1], -np.inf, -0.0, 1, 0.5, 16777216, 1e30]], F32)
    return a


# ---- the host twin and the kernels through the C-ABI ---------------------------------------------------------------------------
def _table(E, R_, V, zone, offset, row, col):
    return dict(E=int(E), ring_zone=zone[:R_].copy(), ring_offset=offset[:R_ + 1].copy(), vertex_row=row[:V].copy(), vertex_col=col[:V].copy())


def host_cabi(A, band, stride=None, offset=0):
    """pcr_hip_polygonize_host on a strided host band between sentinels: the counts first, then the table."""
    L = A.lib()
    h, w = band.shape
    stride = stride or w
    buf, _ = R.strided(np.ascontiguousarray(band, F32), stride, offset)
    E, Rn, V = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    A.check(L.pcr_hip_polygonize_host(buf.ctypes.data + 4 * offset, w, h, stride, C.byref(E), C.byref(Rn), C.byref(V), 0, 0, None, None, None, None))
    zone, off = np.full(Rn.value + 1, 0xEEEEEEEE, U32), np.full(Rn.value + 2, -7, I64)
    row, col = np.full(V.value + 1, -7, I32), np.full(V.value + 1, -7, I32)
    if Rn.value:
        A.check(L.pcr_hip_polygonize_host(buf.ctypes.data + 4 * offset, w, h, stride, None, None, None, Rn.value, V.value, zone.ctypes.data,
                                          off.ctypes.data, row.ctypes.data, col.ctypes.data))
        assert zone[-1] == 0xEEEEEEEE and off[-1] == -7 and row[-1] == -7 and col[-1] == -7, "the twin wrote past the table"
    else:
        off[0] = 0
    return _table(E.value, Rn.value, V.value, zone, off, row, col)


def device_cabi(A, band, stride=None, offset=0):
    """The kernels on a strided device band between sentinels.  -> (table, key rounds worked, rank rounds worked)."""
    L = A.lib()
    h, w = band.shape
    stride = stride or w
    buf, _ = R.strided(np.ascontiguousarray(band, F32), stride, offset)
    d_band = A.DeviceBuffer.from_numpy(buf)
    ptr = d_band.ptr.value + 4 * offset
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_polygonize_cells_work_bytes(w, h, C.byref(nbytes)))
    d_cells = A.DeviceBuffer(nbytes.value)
    A.check(L.pcr_hip_polygonize_edges(ptr, w, h, stride, d_cells.ptr, nbytes.value, None))
    E, Rn, V, kr, rr = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int(-1), C.c_int(-1)
    A.check(L.pcr_hip_polygonize_count(d_cells.ptr, nbytes.value, C.byref(E), None, None, None, None, None))
    if E.value == 0:
        d_band.free()
        d_cells.free()
        return _table(0, 0, 0, np.zeros(0, U32), np.zeros(1, I64), np.zeros(0, I32), np.zeros(0, I32)), 0, 0
    rbytes = C.c_size_t(0)
    A.check(L.pcr_hip_polygonize_rings_work_bytes(E.value, C.byref(rbytes)))
    d_rings = A.DeviceBuffer(rbytes.value)
    A.check(L.pcr_hip_polygonize_rings(ptr, w, h, stride, d_cells.ptr, nbytes.value, E.value, d_rings.ptr, rbytes.value, None, None))
    A.check(L.pcr_hip_polygonize_count(d_cells.ptr, nbytes.value, C.byref(E), C.byref(Rn), C.byref(V), C.byref(kr), C.byref(rr), None))
    assert 1 <= Rn.value and 4 * Rn.value <= V.value <= E.value, (E.value, Rn.value, V.value)
    d_zone = A.DeviceBuffer.from_numpy(np.full(Rn.value + 1, 0xEEEEEEEE, U32))
    d_off = A.DeviceBuffer.from_numpy(np.full(Rn.value + 2, -7, I64))
    d_row = A.DeviceBuffer.from_numpy(np.full(V.value + 1, -7, I32))
    d_col = A.DeviceBuffer.from_numpy(np.full(V.value + 1, -7, I32))
    A.check(L.pcr_hip_polygonize_fetch(ptr, w, h, stride, d_cells.ptr, nbytes.value, E.value, d_rings.ptr, rbytes.value, Rn.value, V.value,
                                       d_zone.ptr, d_off.ptr, d_row.ptr, d_col.ptr, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    zone, off = d_zone.to_numpy(U32, (Rn.value + 1,)), d_off.to_numpy(I64, (Rn.value + 2,))
    row, col = d_row.to_numpy(I32, (V.value + 1,)), d_col.to_numpy(I32, (V.value + 1,))
    assert zone[-1] == 0xEEEEEEEE and off[-1] == -7 and row[-1] == -7 and col[-1] == -7, "a kernel wrote past the table"
    R.sentinels_survive(d_band.to_numpy(F32, buf.shape), w, h, stride, offset)
    for d in (d_band, d_cells, d_rings, d_zone, d_off, d_row, d_col):
        d.free()
    return _table(E.value, Rn.value, V.value, zone, off, row, col), kr.value, rr.value


def make_grid(pcr, band, g=None, name="zones"):
    h, w = band.shape
    d = pcr.BandDesc()
    d.name = name
    grid = pcr.Grid.create(w, h, [d])
    grid.set_band_array(0, np.ascontiguousarray(band, F32))
    if g is not None:
        grid.set_geometry(g.config())
    return grid
