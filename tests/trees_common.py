"""Shared by tests/test_trees.py and tests/test_gpu_trees.py: the brute-force model of the tree bands (the contract of
csrc/trees.hpp) -- no engine code: plain loops over cells, every disc scanned, dict parents, chains walked -- the canopy
generator, and the ways the tests reach the host twin and the kernels."""
import ctypes as C
import math

import numpy as np

import ground_filter_common as G
import overviews_common as M
import pcr

NAN_BITS = M.NAN_BITS
make_grid, grid_bands, bits_equal = M.make_grid, M.grid_bands, M.bits_equal
F32, F64 = np.float32, np.float64
COLUMNS = ("row", "col", "x", "y", "height", "crown_cells")
DEFAULTS = dict(min_height=2.0, window_base=3.0, window_slope=0.07, max_radius_cells=16, min_crown_height=2.0, crown_ratio=0.45,
                max_crown_radius=10.0)


def spec(**kw):
    s = pcr.TreeSpec()
    for k, v in kw.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    return s


def nan32():
    return np.array([NAN_BITS], np.uint32).view(F32)[0]


def model(src, cell_size_x=1.0, cell_size_y=-1.0, **kw):
    """-> dict(id, height: float32 [h, w]; table: dict of arrays; step3: cells that took parent step 3; labelled: their number)."""
    p = dict(DEFAULTS)
    p.update(kw)
    H = np.ascontiguousarray(src, F32)
    h, w = H.shape
    min_height, min_crown, ratio = F32(p["min_height"]), F32(p["min_crown_height"]), F32(p["crown_ratio"])
    base, slope, max_r = F64(F32(p["window_base"])), F64(F32(p["window_slope"])), int(p["max_radius_cells"])
    cell = max(abs(float(cell_size_x)), abs(float(cell_size_y)))
    k = F64(0.5) / F64(cell)
    mcr = F32(p["max_crown_radius"])
    Mc = -1 if np.isinf(mcr) else int(min(math.floor(float(F64(mcr) / F64(cell))), 2 ** 31 - 1))
    data = np.isfinite(H)

    def beats(a, b):                                     # cells as (r, c)
        ha, hb = H[a], H[b]
        return bool(ha > hb) or (bool(ha == hb) and a[0] * w + a[1] < b[0] * w + b[1])

    def radius(c):
        d = base + slope * F64(H[c])
        rho = d * k
        if rho >= max_r:
            return max_r
        if not rho >= 1.0:
            return 0
        return int(rho)

    def best(c):
        R = radius(c)
        b = c
        for dr in range(-R, R + 1):
            for dc in range(-R, R + 1):
                q = (c[0] + dr, c[1] + dc)
                if dr * dr + dc * dc <= R * R and 0 <= q[0] < h and 0 <= q[1] < w and data[q] and beats(q, b):
                    b = q
        return b

    cells = [(r, c) for r in range(h) for c in range(w) if data[r, c]]
    bests = {c: best(c) for c in cells}
    tops = [c for c in cells if H[c] >= min_height and bests[c] == c]          # in idx order
    ids = {c: i + 1 for i, c in enumerate(tops)}
    parent, step3 = {}, []
    for c in cells:
        if c in ids:
            parent[c] = c
            continue
        if not H[c] >= min_crown:
            continue
        nb = None
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                q = (c[0] + dr, c[1] + dc)
                if (dr or dc) and 0 <= q[0] < h and 0 <= q[1] < w and data[q] and beats(q, c) and (nb is None or beats(q, nb)):
                    nb = q
        if nb is None:
            step3.append(c)
            nb = bests[c]
        parent[c] = nb
    out_id = np.full((h, w), nan32(), F32)
    out_h = np.full((h, w), nan32(), F32)
    crown = [0] * len(tops)
    chain = 0
    for c in parent:
        root, n = c, 0
        while parent[root] != root:
            root, n = parent[root], n + 1
        chain = max(chain, n)
        if root not in ids:
            continue
        if c != root:
            if not H[c] >= ratio * H[root]:              # one float32 multiplication
                continue
            dr, dc = c[0] - root[0], c[1] - root[1]
            if Mc >= 0 and dr * dr + dc * dc > Mc * Mc:
                continue
        crown[ids[root] - 1] += 1
        if ids[root] <= 2 ** 24:
            out_id[c] = F32(ids[root])
            out_h[c] = H[root]
    csx, csy = float(cell_size_x), float(cell_size_y)
    table = dict(row=np.array([t[0] for t in tops], np.int32), col=np.array([t[1] for t in tops], np.int32),
                 x=np.array([(t[1] + 0.5) * csx for t in tops], F64), y=np.array([(t[0] + 0.5) * csy for t in tops], F64),
                 height=np.array([H[t] for t in tops], F32), crown_cells=np.array(crown, np.int32))
    return dict(id=out_id, height=out_h, table=table, step3=step3, labelled=int(sum(crown)), chain=chain)


def canopy(w, h, seed):
    """A canopy height model: Gaussian bumps of height 3..30 and sigma 1..4 cells, about one per 60 cells, combined by maximum;
    noise of sigma 0.3; rounded to 0.25 so that ties abound; 5 % NaN; a few +-Inf cells."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:h, 0:w]
    z = np.zeros((h, w), F64)
    for _ in range(max(1, w * h // 60)):
        r0, c0 = rng.uniform(0, h), rng.uniform(0, w)
        a, s = rng.uniform(3.0, 30.0), rng.uniform(1.0, 4.0)
        z = np.maximum(z, a * np.exp(-((rr - r0) ** 2 + (cc - c0) ** 2) / (2.0 * s * s)))
    z = z + rng.normal(0.0, 0.3, (h, w))
    z = (np.round(z * 4.0) / 4.0).astype(F32)
    z[rng.random((h, w)) < 0.05] = np.nan
    for _ in range(min(6, w * h // 8)):
        z[rng.integers(0, h), rng.integers(0, w)] = np.inf if rng.random() < 0.5 else -np.inf
    return z


def exercises_the_rules(src, m):
    """What every test of a generated field first asserts of the MODEL's result."""
    assert len(m["table"]["row"]) >= 100, len(m["table"]["row"])
    assert len(m["step3"]) >= 3, len(m["step3"])
    assert m["labelled"] >= 1000, m["labelled"]
    a = np.ascontiguousarray(src, F32)
    with np.errstate(all="ignore"):
        ties = (a[:, 1:] == a[:, :-1]).sum() + (a[1:, :] == a[:-1, :]).sum() + (a[1:, 1:] == a[:-1, :-1]).sum() + (a[1:, :-1] == a[:-1, 1:]).sum()
    assert ties >= 1


def same_result(got, want, what=""):
    """Both bands bit for bit (NaNs included: every NaN made is 0x7FC00000) and every column of the table."""
    bits_equal(got["id"], want["id"], what + " tree_id")
    bits_equal(got["height"], want["height"], what + " tree_height")
    for k in COLUMNS:
        if k not in got["table"] or k not in want["table"]:      # (the C-ABI knows no centres)
            continue
        a, b = np.asarray(got["table"][k]), np.asarray(want["table"][k])
        assert a.shape == b.shape, f"{what} table.{k}: {a.shape} != {b.shape}"
        assert a.dtype == b.dtype, f"{what} table.{k}: {a.dtype} != {b.dtype}"
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what} table.{k} differs"


# ---- the host twin -----------------------------------------------------------------------------------------------------------
def host(src, sp=None, cell_size_x=1.0, cell_size_y=-1.0):
    from pcr import _pcr
    i, hh, t = _pcr._trees_host(np.ascontiguousarray(src, F32), sp, cell_size_x, cell_size_y)
    return dict(id=np.array(i), height=np.array(hh), table={k: np.array(v) for k, v in t.items()})


SENTINEL = F32(-12345.5)


def strided(a, stride, offset=0):
    """(buffer, view): `a` inside a float32 buffer of SENTINELs with rows `stride` floats apart, `offset` floats in."""
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


def params(A, cell_size_x=1.0, cell_size_y=-1.0, **kw):
    return A.TreeParams(cell_size_x=cell_size_x, cell_size_y=cell_size_y, **kw)


def host_cabi(A, src, stride=None, cell_size_x=1.0, cell_size_y=-1.0, want_height=True, **kw):
    """pcr_hip_trees_host on strided host arrays between sentinels."""
    L = A.lib()
    a = np.ascontiguousarray(src, F32)
    h, w = a.shape
    stride = stride or w
    sbuf, sview = strided(a, stride)
    ibuf, iview = strided(np.zeros((h, w), F32), stride)
    hbuf, hview = strided(np.zeros((h, w), F32), stride)
    cap = w * h
    rows, cols, crown = (np.zeros(cap, np.int32) for _ in range(3))
    heights = np.zeros(cap, F32)
    n = C.c_int64(-1)
    p = params(A, cell_size_x, cell_size_y, **kw)
    A.check(L.pcr_hip_trees_host(sbuf.ctypes.data, w, h, stride, C.byref(p), ibuf.ctypes.data, stride,
                                 hbuf.ctypes.data if want_height else None, stride, C.byref(n), cap, rows.ctypes.data,
                                 cols.ctypes.data, heights.ctypes.data, crown.ctypes.data))
    bits_equal(sview, a, "src is only read")
    for b in (sbuf, ibuf, hbuf):
        sentinels_survive(b, w, h, stride)
    T = n.value
    return dict(id=iview.copy(), height=hview.copy() if want_height else None,
                table=dict(row=rows[:T].copy(), col=cols[:T].copy(), height=heights[:T].copy(), crown_cells=crown[:T].copy()))


# ---- the kernels -------------------------------------------------------------------------------------------------------------
def device_cabi(A, src, stride=None, offset=0, cell_size_x=1.0, cell_size_y=-1.0, want_height=True, **kw):
    """pcr_hip_trees, _count and _table on strided device arrays between sentinels; -> result, rounds that did work."""
    L = A.lib()
    a = np.ascontiguousarray(src, F32)
    h, w = a.shape
    stride = stride or w
    sbuf, _ = strided(a, stride, offset)
    ibuf, _ = strided(np.zeros((h, w), F32), stride, offset)
    hbuf, _ = strided(np.zeros((h, w), F32), stride, offset)
    d_src, d_id, d_h = (A.DeviceBuffer.from_numpy(b) for b in (sbuf, ibuf, hbuf))
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_trees_work_bytes(w, h, C.byref(nbytes)))
    d_work = A.DeviceBuffer(nbytes.value)
    p = params(A, cell_size_x, cell_size_y, **kw)
    at = lambda d: d.ptr.value + 4 * offset
    A.check(L.pcr_hip_trees(at(d_src), w, h, stride, C.byref(p), at(d_id), stride, at(d_h) if want_height else None, stride,
                            d_work.ptr, nbytes.value, None))
    n, rounds = C.c_int64(-1), C.c_int(-1)
    A.check(L.pcr_hip_trees_count(d_work.ptr, nbytes.value, C.byref(n), C.byref(rounds), None))
    T = n.value
    d_cols = [A.DeviceBuffer(max(T, 1) * 4) for _ in range(4)]
    A.check(L.pcr_hip_trees_table(at(d_src), w, h, stride, d_work.ptr, nbytes.value, T, *[d.ptr for d in d_cols], None))
    A.check(L.pcr_hip_stream_synchronize(None))
    out_s, out_i, out_h = (d.to_numpy(F32, b.shape) for d, b in ((d_src, sbuf), (d_id, ibuf), (d_h, hbuf)))
    assert np.array_equal(out_s.view(np.uint32), sbuf.view(np.uint32)), "src is only read"
    for b in (out_i, out_h):
        sentinels_survive(b, w, h, stride, offset)
    view = lambda b: np.lib.stride_tricks.as_strided(b[offset:], (h, w), (4 * stride, 4)).copy()
    dt = (np.int32, np.int32, F32, np.int32)
    row, col, height, crown = (d.to_numpy(t, (max(T, 1),))[:T] for d, t in zip(d_cols, dt))
    for d in [d_src, d_id, d_h, d_work] + d_cols:
        d.free()
    return dict(id=view(out_i), height=view(out_h) if want_height else None,
                table=dict(row=row, col=col, height=height, crown_cells=crown)), rounds.value


# ---- the pipelines' common ground --------------------------------------------------------------------------------------------
def band_cfg(source, id_name="", height_name="", **kw):
    t = pcr.TreeBandConfig()
    t.source_band, t.id_band_name, t.height_band_name = source, id_name, height_name
    for k, v in kw.items():
        assert hasattr(t, k), k
        setattr(t, k, v)
    return t


def spec_of(t):
    return spec(**{k: getattr(t, k) for k in DEFAULTS})


def canopy_cloud(W, H, seed):
    """One point per cell at its centre, the canopy's value as the channel `value` (cells without data get no point), and the
    band a Max of it is."""
    z = canopy(W, H, seed)
    z[~np.isfinite(z)] = np.nan
    z[z == 0.0] = 0.0                                     # (the engines' Min and Max of -0.0 and +0.0 need not agree on the sign)
    rr, cc = np.nonzero(~np.isnan(z))
    c = pcr.PointCloud.create(len(rr))
    c.set_x_array(cc + 0.5)
    c.set_y_array(H - (rr + 0.5))
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", z[rr, cc].astype(F32))
    return c, z


pipeline_cfg = G.pipeline_cfg
