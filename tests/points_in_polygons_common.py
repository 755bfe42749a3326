"""Shared by tests/test_points_in_polygons.py and tests/test_gpu_points_in_polygons.py: the brute-force model of the exact
point-in-polygon test (the contract of csrc/point_in_polygon.hpp) -- no engine code and no index: every point against every edge
of every polygon in NumPy float64, which does no FMA -- the polygon sets, the point lattice, and the ways the tests reach the
host twin and the kernel."""
import ctypes as C

import numpy as np

import rasterize_common as RC
from rasterize_common import F32, F64, Polys, bits_equal, nan32  # noqa: F401

SENTINEL = RC.SENTINEL
INDEX_SIZES = ((1, 1), (2, 3), (7, 5), (64, 64), (0, 0))         # (index_cols, index_rows); (0, 0): automatic


# ---- the model -------------------------------------------------------------------------------------------------------------------
def edges_of(polys, p):
    """The edges of polygon p, ordered a.y <= b.y: (ax, ay, bx, by) float64 arrays."""
    out = []
    for ring in polys.polygon(p):
        a, b = ring, np.roll(ring, -1, axis=0)
        swap = a[:, 1] > b[:, 1]
        lo, hi = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
        out.append(np.concatenate([lo, hi], axis=1))
    e = np.concatenate(out) if out else np.zeros((0, 4))
    return e[:, 0], e[:, 1], e[:, 2], e[:, 3]


def inside(polys, p, x, y):
    """Which of the points polygon p holds: the parity of its crossing edges with xc > x."""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    odd = np.zeros(x.shape, bool)
    ax, ay, bx, by = edges_of(polys, p)
    with np.errstate(all="ignore"):
        for e in range(len(ax)):
            crosses = (ay[e] <= y) & (y < by[e])
            t = (y - ay[e]) / (by[e] - ay[e])
            xc = ax[e] + t * (bx[e] - ax[e])
            odd ^= crosses & (xc > x)
    return odd


def model(polys, x, y, background=None):
    """Float32 per point: the value of the greatest-index polygon that holds it, the background elsewhere."""
    bg = nan32() if background is None else background
    out = np.full(len(x), bg, F32)
    for p in range(polys.P):                                      # ascending: a later polygon over an earlier
        value = F32(p + 1) if polys.values is None else polys.values[p]
        out[inside(polys, p, x, y)] = value
    return out


# ---- polygon sets ----------------------------------------------------------------------------------------------------------------
def rectangles():
    """Axis-parallel rectangles: horizontal edges through index cells, sides on round numbers, one inside another."""
    return Polys([[RC.rect(2.0, 3.0, 40.0, 29.0)], [RC.rect(10.0, 8.0, 20.0, 16.0)], [RC.rect(40.0, 3.0, 64.0, 29.0)],
                  [RC.rect(-5.5, 29.0, 17.25, 48.0)]])


def donut():
    return Polys([RC.donut(30.0, 30.0, 22.0, 9.0)])


def comb():
    return Polys([[RC.comb(1.0, 2.0, teeth=17)]])


def ngons(count=300, seed=7):
    rng = np.random.default_rng(seed)
    polys = [[RC.ngon(rng.uniform(0, 200), rng.uniform(0, 150), rng.uniform(2, 40), int(rng.integers(3, 13)), rng.uniform(0, 1))]
             for _ in range(count)]
    return Polys(polys, rng.uniform(-50, 50, count).astype(F32))


def jittered_partition():
    return Polys(RC.partition(5.0, -7.0, 95.0, 61.0, 5, 4, seed=3))


def far_triangle():
    """A triangle with one vertex far outside the others: long edges that every column's band list holds."""
    return Polys([[np.array([[0.0, 0.0], [10.0, 1.0], [1.0e7, 3.0e6]])], [RC.ngon(5.0, 0.6, 0.5, 5)]])


def degenerate():
    """A polygon without a ring, one without area (three collinear points, and a ring walked forth and back), a horizontal
    sliver of no height, between two ordinary ones."""
    return Polys([[RC.rect(0.0, 0.0, 8.0, 8.0)], [], [np.array([[1.0, 1.0], [3.0, 3.0], [5.0, 5.0]])],
                  [np.array([[1.0, 2.0], [6.0, 2.0], [3.0, 2.0]])], [np.array([[0.0, 5.0], [4.0, 7.0], [0.0, 5.0], [4.0, 7.0]])],
                  [RC.ngon(9.0, 9.0, 3.0, 7)]])


def big_ngon(n=1000):
    return Polys([[RC.ngon(50.0, 50.0, 40.0, n)]])


SETS = {"rectangles": rectangles, "donut": donut, "comb": comb, "ngons": ngons, "partition": jittered_partition,
        "far_triangle": far_triangle, "degenerate": degenerate}


# ---- the point lattice -----------------------------------------------------------------------------------------------------------
def _around(v):
    v = np.asarray(v, F64)
    return np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])


def boundaries(lo, hi, g, most=24):
    """The nominal boundaries of g index cells over [lo, hi] (at most `most` of them, the ends among them), one ulp either side."""
    if g <= 1 or not hi > lo:
        return _around(np.array([lo, hi]))
    ks = np.unique(np.round(np.linspace(0, g, min(g + 1, most))).astype(int))
    return _around(np.concatenate([lo + ks * ((hi - lo) / g), lo + (hi - lo) * (ks / g)]))


def lattice(polys, index_shapes=()):
    """Every vertex; every edge's midpoint; each of those one nextafter either side in x and in y; the cell boundaries of every
    index shape one ulp either side (crossed with each other); points far outside on all four sides; NaN and +-Inf in either
    coordinate; and 1500 points spread uniformly over the bounding box and a margin, for the cells no edge is near."""
    v = polys.coords
    mids = []
    for p in range(polys.P):
        for ring in polys.polygon(p):
            mids.append((ring + np.roll(ring, -1, axis=0)) / 2.0)
    pts = np.concatenate([v] + mids) if len(v) else np.zeros((0, 2))
    xs, ys = [pts[:, 0]], [pts[:, 1]]
    for d in (-np.inf, np.inf):
        xs += [np.nextafter(pts[:, 0], d), pts[:, 0]]
        ys += [pts[:, 1], np.nextafter(pts[:, 1], d)]
    x0, x1 = (v[:, 0].min(), v[:, 0].max()) if len(v) else (0.0, 1.0)
    y0, y1 = (v[:, 1].min(), v[:, 1].max()) if len(v) else (0.0, 1.0)
    for gx, gy in index_shapes:
        bx, by = boundaries(x0, x1, gx), boundaries(y0, y1, gy)
        inner_x = np.concatenate([bx, x0 + (x1 - x0) * np.array([0.123, 0.5, 0.871])])
        inner_y = np.concatenate([by, y0 + (y1 - y0) * np.array([0.317, 0.5, 0.93])])
        gxs, gys = np.meshgrid(inner_x, inner_y)
        xs.append(gxs.ravel())
        ys.append(gys.ravel())
    w, h = max(x1 - x0, 1.0), max(y1 - y0, 1.0)
    mx, my = (x0 + x1) / 2, (y0 + y1) / 2
    far = [(x0 - 10 * w, my), (x1 + 10 * w, my), (mx, y0 - 10 * h), (mx, y1 + 10 * h), (-1e300, my), (1e300, my), (mx, -1e300), (mx, 1e300),
           (x0 - 10 * w, y0 - 10 * h), (x1 + 10 * w, y1 + 10 * h)]
    special = [(np.nan, my), (mx, np.nan), (np.nan, np.nan), (np.inf, my), (-np.inf, my), (mx, np.inf), (mx, -np.inf), (np.inf, np.inf),
               (-np.inf, -np.inf), (np.nan, np.inf), (-np.inf, np.nan), (x0, np.nan), (np.nan, y0)]
    extra = np.array(far + special, F64)
    xs.append(extra[:, 0])
    ys.append(extra[:, 1])
    rng = np.random.default_rng(len(v))                           # and the inner points of the cells: a uniform spread
    xs.append(rng.uniform(x0 - 0.1 * w, x1 + 0.1 * w, 1500))
    ys.append(rng.uniform(y0 - 0.1 * h, y1 + 0.1 * h, 1500))
    return np.ascontiguousarray(np.concatenate(xs), F64), np.ascontiguousarray(np.concatenate(ys), F64)


# ---- the host twin and the kernel through the C-ABI ----------------------------------------------------------------------------
class Index:
    """pcr_hip_polygon_index_create ... _destroy around a Polys."""

    def __init__(self, A, polys, cols=0, rows=0, background_bits=None, max_index_bytes=0):
        self.A, self.L, self.polys = A, A.lib(), polys
        self.ptr = C.c_void_p()
        p = A.PolygonIndexParams(index_cols=cols, index_rows=rows, max_index_bytes=max_index_bytes)
        if background_bits is not None:                           # (through memory: a float argument may quieten a payload)
            C.memmove(C.byref(p), np.array([background_bits], np.uint32).ctypes.data, 4)
        self.params = p
        A.check(self.L.pcr_hip_polygon_index_create(*poly_args(polys), C.byref(p), C.byref(self.ptr)))
        self.d_tables = None

    def info(self):
        cols, rows, items, listed, nbytes = C.c_int(), C.c_int(), C.c_int64(), C.c_int64(), C.c_size_t()
        self.A.check(self.L.pcr_hip_polygon_index_info(self.ptr, C.byref(cols), C.byref(rows), C.byref(items), C.byref(listed),
                                                       C.byref(nbytes)))
        return dict(cols=cols.value, rows=rows.value, items=items.value, listed_edges=listed.value, bytes=nbytes.value)

    def host(self, x, y, threads=1):
        out = np.full(len(x) + 2, SENTINEL, F32)
        self.A.check(self.L.pcr_hip_points_in_polygons_host(self.ptr, x.ctypes.data, y.ctypes.data, len(x), out.ctypes.data + 4, threads))
        assert out[0] == SENTINEL and out[-1] == SENTINEL
        return out[1:-1].copy()

    def upload(self):
        nbytes = self.info()["bytes"]
        self.d_tables = self.A.DeviceBuffer(nbytes)
        self.A.check(self.L.pcr_hip_polygon_index_upload(self.ptr, self.d_tables.ptr, nbytes, None))
        return self

    def device(self, x, y, off_x=0, off_y=0, off_out=0):
        """The kernel on x, y and out that start `off` elements into their buffers (0: on 16 bytes), out between sentinels."""
        A, n = self.A, len(x)
        if self.d_tables is None:
            self.upload()
        hx, hy = np.zeros(n + off_x + 2, F64), np.zeros(n + off_y + 2, F64)
        hx[off_x:off_x + n], hy[off_y:off_y + n] = x, y
        hout = np.full(n + off_out + 8, SENTINEL, F32)
        dx, dy, dout = A.DeviceBuffer.from_numpy(hx), A.DeviceBuffer.from_numpy(hy), A.DeviceBuffer.from_numpy(hout)
        A.check(self.L.pcr_hip_points_in_polygons(self.ptr, self.d_tables.ptr, dx.ptr.value + 8 * off_x, dy.ptr.value + 8 * off_y, n,
                                                  dout.ptr.value + 4 * off_out, None, None))
        A.check(self.L.pcr_hip_stream_synchronize(None))
        got = dout.to_numpy(F32, hout.shape)
        for b in (dx, dy, dout):
            b.free()
        keep = np.ones(len(got), bool)
        keep[off_out:off_out + n] = False
        assert (got[keep].view(np.uint32) == np.array([SENTINEL], F32).view(np.uint32)[0]).all(), "a slot outside the output was written"
        return got[off_out:off_out + n].copy()

    def close(self):
        if self.d_tables is not None:
            self.d_tables.free()
            self.d_tables = None
        if self.ptr:
            self.L.pcr_hip_polygon_index_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def poly_args(polys, **over):
    ptr = lambda a: None if a is None else a.ctypes.data
    a = (ptr(polys.coords), len(polys.coords), ptr(polys.ring_offsets), len(polys.ring_offsets) - 1, ptr(polys.polygon_offsets), polys.P,
         ptr(polys.values))
    names = ("coords", "V", "ring_offsets", "R", "polygon_offsets", "P", "values")
    return tuple(over.get(n, v) for n, v in zip(names, a))


def create_error(A, polys, params=None, index_out=True, **over):
    """The return code and message of a pcr_hip_polygon_index_create that is expected to be refused."""
    L = A.lib()
    ptr = C.c_void_p()
    p = params if params is not None else A.PolygonIndexParams()
    rc = L.pcr_hip_polygon_index_create(*poly_args(polys, **over), C.byref(p) if p != "null" else None,
                                        C.byref(ptr) if index_out else None)
    msg = L.pcr_hip_last_error().decode()
    if rc == 0:
        L.pcr_hip_polygon_index_destroy(ptr)
    return rc, msg


# ---- pipelines: "derived at ingest == the model's channel precomputed", bit for bit ---------------------------------------------
def plots():
    """Plots over the pipeline grid of sample_grid_common (40 x 24): a partition of [3, 35] x [2, 21] with vertices on eighths
    where the points are, a donut over it, a rectangle half outside the grid."""
    parts = RC.partition(3.0, 2.0, 35.0, 21.0, 4, 3, seed=9)
    parts = [[np.round(r * 8.0) / 8.0 for r in rings] for rings in parts]
    return Polys(parts + [RC.donut(20.0, 12.0, 6.0, 2.5), [RC.rect(33.5, 17.25, 44.0, 30.0)]])


def plot_points(n, seed):
    import sample_grid_common as SG
    return SG.dyadic_points(n, seed)


def with_plot(c, polys, name="plot", background=None, x=None, y=None):
    """The cloud dict with the model's channel added (taken at x, y when given: the reprojected coordinates)."""
    out = dict(c)
    out[name] = model(polys, c["x"] if x is None else x, c["y"] if y is None else y, background)
    return out


def polygon_pipeline(pcr, make_config, specs, cfg_filt=(), names=("plot",), **kw):
    p = pcr.Pipeline.create(make_config(specs, cfg_filt, polygon_channels=[pcr.PolygonChannelConfig(n) for n in names], **kw))
    assert p is not None, pcr.pipeline_create_error()
    return p


def plain_pipeline(pcr, make_config, specs, cfg_filt=(), **kw):
    q = pcr.Pipeline.create(make_config(specs, cfg_filt, **kw))
    assert q is not None, pcr.pipeline_create_error()
    return q


def check_clip_and_counts(pcr, make_config, location=None, what=""):
    """The exact clip (cfg.filter on the channel), a Count per plot, the channel as a value; against the precomputed channel and
    against NumPy's count of the model's labels.  -> the bands of both configurations, for a comparison across engines."""
    import reduction_filters_common as RF
    import sample_grid_common as SG
    S = RF.S
    polys = plots()
    c = plot_points(5000, 21)
    pre = with_plot(c, polys)
    ks = (1.0, 6.0, 13.0, 14.0)
    specs = [S("Count", ch="z", filt=[("plot", "Equal", k)]) for k in ks] + [S("Max", ch="plot"), S("Sum", ch="plot"), S("Count", ch="z")]
    every = []
    for cfg_filt in ((), [("plot", "GreaterEqual", 1.0)]):
        p, q = polygon_pipeline(pcr, make_config, specs, cfg_filt), plain_pipeline(pcr, make_config, specs, cfg_filt)
        p.set_polygons("plot", polys.to_pcr())
        p.ingest(SG.dict_cloud(pcr, c, location))
        q.ingest(SG.dict_cloud(pcr, pre, location))
        p.finalize()
        q.finalize()
        bands = SG.assert_same_pipelines(p, q, f"{what}: filter {cfg_filt}")
        every += bands
        inside = RF.cells_of(SG.PGRID, c["x"], c["y"]) >= 0      # (the points that the grid routes to a cell at all)
        for k, band in zip(ks, bands):
            want = int(((pre["plot"] == k) & inside).sum())
            assert want > 20 and int(np.nansum(band)) == want, (k, want, float(np.nansum(band)))
        if cfg_filt:                                              # the clip: what is counted at all is what some plot holds
            assert int(np.nansum(bands[-1])) == int(((pre["plot"] >= 1.0) & inside).sum()) < int(inside.sum())
    return every


def check_histogram(pcr, make_config, location=None):
    import histogram_common as HC
    import reduction_filters_common as RF
    import sample_grid_common as SG
    polys, c = plots(), plot_points(3000, 5)
    hist = [HC.histogram(pcr, "plot", 0.5, 14.5, 14)]
    p = polygon_pipeline(pcr, make_config, [RF.S("Count", ch="z")], histograms=hist)
    q = plain_pipeline(pcr, make_config, [RF.S("Count", ch="z")], histograms=hist)
    p.set_polygons("plot", polys.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c, location))
    q.ingest(SG.dict_cloud(pcr, with_plot(c, polys), location))
    got, want = np.asarray(p.histogram(0)), np.asarray(q.histogram(0))
    assert got.shape == want.shape and (got == want).all() and int(got.sum()) > 1000
    p.finalize()
    q.finalize()
    SG.assert_same_pipelines(p, q, "histogram of the channel")


def check_set_polygons_again(pcr, make_config, location=None):
    """Two ingests with other polygons, another background and another index size between them."""
    import reduction_filters_common as RF
    import sample_grid_common as SG
    S = RF.S
    specs = [S("Sum", ch="plot"), S("Count", ch="z", filt=[("plot", "Equal", 2.0)]), S("Min", ch="plot")]
    first, second = plots(), Polys([[RC.ngon(12.0, 9.0, 7.5, 9)], [RC.rect(20.0, 4.0, 31.0, 19.0)]])
    c1, c2 = plot_points(2500, 31), plot_points(2500, 32)
    p, q = polygon_pipeline(pcr, make_config, specs), plain_pipeline(pcr, make_config, specs)
    p.set_polygons("plot", first.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c1, location))
    p.set_polygons("plot", second.to_pcr(), background=-1.0, index_cols=7, index_rows=5)
    p.ingest(SG.dict_cloud(pcr, c2, location))
    q.ingest(SG.dict_cloud(pcr, with_plot(c1, first), location))
    q.ingest(SG.dict_cloud(pcr, with_plot(c2, second, background=F32(-1.0)), location))
    p.finalize()
    q.finalize()
    return SG.assert_same_pipelines(p, q, "set_polygons between ingests")


def las_tile(tmp_path):
    """A LAS file over the pipeline grid (coordinates multiples of 1/8): (path, the cloud dict)."""
    import os

    import las_common as LC
    n, fmt = 3000, 1
    rng = np.random.default_rng(23)
    f = LC.make_fields(fmt, n, rng)
    f["X"] = rng.integers(-8, 8 * 40 + 9, n).astype(np.int32)
    f["Y"] = rng.integers(-8, 8 * 24 + 9, n).astype(np.int32)
    f["Z"] = rng.integers(0, 512, n).astype(np.int32)
    scale, offset = (0.125, 0.125, 0.125), (0.0, 0.0, 0.0)
    path = os.path.join(str(tmp_path), "tile.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset)
    want = LC.expected(fmt, f, scale, offset)
    return path, dict(x=want["x"], y=want["y"], z=want["z"])


def check_chunked_file(pcr, make_config, tmp_path):
    import reduction_filters_common as RF
    import sample_grid_common as SG
    S = RF.S
    path, c = las_tile(tmp_path)
    polys = plots()
    specs = [S("Count", ch="z", filt=[("plot", "Equal", 6.0)]), S("Sum", ch="plot"), S("Max", ch="z")]
    clip = [("plot", "GreaterEqual", 1.0)]
    p, q = polygon_pipeline(pcr, make_config, specs, clip), plain_pipeline(pcr, make_config, specs, clip)
    p.set_polygons("plot", polys.to_pcr())
    assert p.ingest_file(path, 700) == len(c["x"])              # five chunks; the file is never asked for `plot`
    q.ingest(SG.dict_cloud(pcr, with_plot(c, polys)))
    p.finalize()
    q.finalize()
    SG.assert_same_pipelines(p, q, "chunked ingest_file", collections=False)


def check_reprojected(pcr, mode_name, location=None):
    """A cloud in EPSG:4326 into a UTM grid with polygons in UTM: the channel is taken at the reprojected coordinates."""
    import reduction_filters_common as RF
    import reproject_common as RPC
    import sample_grid_common as SG
    S = RF.S
    size = 24
    mode = pcr.ExecutionMode.CPU if mode_name == "cpu" else pcr.ExecutionMode.GPU

    def config(specs, cfg_filt=(), **kw):
        cfg = RPC.make_config(pcr, size, mode)
        cfg.reductions = [RF.to_spec(s) for s in specs]
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg
    b = RPC.grid_bounds(size)
    w, h = b[2] - b[0], b[3] - b[1]
    polys = Polys(RC.partition(b[0] + 0.1 * w, b[1] + 0.15 * h, b[0] + 0.8 * w, b[1] + 0.9 * h, 3, 2, seed=4)
                  + [[RC.ngon(b[0] + 0.5 * w, b[1] + 0.5 * h, 0.2 * min(w, h), 11)]])
    x, y, v = RPC.cell_points(size, 4000, seed=5)
    lon, lat = pcr.transform_xy(RPC.GRID_EPSG, 4326, x, y)
    c = dict(x=lon, y=lat, z=(v * 60.0).astype(F32))
    crs_deg, crs_utm = pcr.CRS.from_epsg(4326), pcr.CRS.from_epsg(RPC.GRID_EPSG)
    specs = [S("Count", ch="z", filt=[("plot", "Equal", 7.0)]), S("Sum", ch="plot"), S("Count", ch="z", filt=[("plot", "Equal", 2.0)])]
    p, q = polygon_pipeline(pcr, config, specs), plain_pipeline(pcr, config, specs)
    p.set_polygons("plot", polys.to_pcr())
    p.ingest(SG.dict_cloud(pcr, c, location, crs=crs_deg))
    moved = SG.dict_cloud(pcr, c, crs=crs_deg)
    pcr.reproject(moved, crs_utm)
    mx, my = np.array(moved.x_array()), np.array(moved.y_array())
    pre = with_plot(dict(c, x=mx, y=my), polys)
    assert (pre["plot"] == 7.0).sum() > 50 and (pre["plot"] == 2.0).sum() > 50 and np.isnan(pre["plot"]).sum() > 50
    q.ingest(SG.dict_cloud(pcr, pre, location, crs=crs_utm))
    p.finalize()
    q.finalize()
    SG.assert_same_pipelines(p, q, f"reprojected cloud, {mode_name}")


def check_pipeline_refusals(pcr, mode, make_config):
    import pytest
    import reduction_filters_common as RF
    import sample_grid_common as SG
    S = RF.S
    ch = pcr.PolygonChannelConfig

    def refused(message, chans, **kw):
        cfg = make_config([S("Sum", ch="plot")], polygon_channels=chans, **kw)
        assert pcr.Pipeline.create(cfg) is None
        assert message in pcr.pipeline_create_error(), pcr.pipeline_create_error()
    refused("polygon_channels[1].name is empty", [ch("plot"), ch("")])
    refused("polygon_channels[2].name 'plot' is given twice", [ch("plot"), ch("b"), ch("plot")])
    refused("polygon_channels[0].name 'plot' is also a surface channel", [ch("plot")], surface_channels=[pcr.SurfaceChannelConfig("plot")])
    refused("more than 8 polygon_channels (9 given)", [ch(f"c{k}") for k in range(9)])
    assert pcr.Pipeline.create(make_config([S("Sum", ch="c0")], polygon_channels=[ch(f"c{k}") for k in range(8)])) is not None
    refused("polygon_channels are not supported on a row-block shard", [ch("plot")], shard_row_begin=0, shard_row_end=16)
    if mode == "gpu":
        refused("polygon_channels are not supported on a pipeline that runs out of core", [ch("plot")], gpu_memory_budget=4096)
    p = polygon_pipeline(pcr, make_config, [S("Sum", ch="plot"), S("Count", ch="z")], names=("plot", "stand"))
    polys, c = plots(), plot_points(100, 1)
    with pytest.raises(RuntimeError, match="polygon channel 'plot' has no polygons"):
        p.ingest(SG.dict_cloud(pcr, c))
    with pytest.raises(RuntimeError, match="'nope' names no polygon channel"):
        p.set_polygons("nope", polys.to_pcr())
    bad = pcr.PolygonSet(np.array([[0.0, 0.0], [1.0, np.inf], [1.0, 1.0]]), np.array([0, 3]), np.array([0, 1]))
    with pytest.raises(RuntimeError, match="a coordinate is not finite or beyond 1e100"):
        p.set_polygons("plot", bad)
    with pytest.raises(RuntimeError, match="index_cols and index_rows must be"):
        p.set_polygons("plot", polys.to_pcr(), index_cols=5000)
    p.set_polygons("plot", polys.to_pcr())
    with pytest.raises(RuntimeError, match="polygon channel 'stand' has no polygons"):
        p.ingest(SG.dict_cloud(pcr, c))
    p.set_polygons("stand", polys.to_pcr())
    with pytest.raises(RuntimeError, match="a coordinate is not finite or beyond 1e100"):          # a refused set keeps the old one
        p.set_polygons("stand", bad)
    with pytest.raises(RuntimeError, match="already carries a channel named 'plot'"):
        p.ingest(SG.dict_cloud(pcr, dict(c, plot=c["z"])))
    assert (p.stats().points_processed, p.stats().collections_processed) == (0, 0), "a refused ingest changes no state"
    p.ingest(SG.dict_cloud(pcr, c))
    assert p.stats().collections_processed == 1
    # without polygon_channels the name is a channel like any other, and set_polygons names nothing
    q = plain_pipeline(pcr, make_config, [S("Sum", ch="z")])
    assert list(make_config([S("Sum", ch="z")]).polygon_channels) == []
    with pytest.raises(RuntimeError, match="names no polygon channel"):
        q.set_polygons("plot", polys.to_pcr())
