"""Shared by tests/test_zonal.py and tests/test_gpu_zonal.py: the model of the zonal-table contract (include/pcr_hip.h, "zonal
tables"; csrc/zonal.hpp) -- no engine code: zone_of cell by cell, the sums as Python ints reduced modulo 2^64, the rows in the
contract's operation order with Python floats (binary64, one rounded operation at a time) -- and ctypes drivers of the C-ABI's
kernels and host twins on strided planes and on tables between sentinel words.  Every comparison made with it is on the bits."""
import ctypes as C
import math

import numpy as np

F32, F64 = np.float32, np.float64
U32, I64, U64 = np.uint32, np.int64, np.uint64
NAN_BITS = 0x7FC00000
M64 = (1 << 64) - 1
MAX_ZONE = 1 << 24
SENTINEL = 0xA5A5A5A5A5A5A5A5
GUARD = 3                                    # sentinel words on either side of a table


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    a, b = got.view(np.uint8).reshape(-1), want.view(np.uint8).reshape(-1)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(got.reshape(-1).view(f"u{got.itemsize}") != want.reshape(-1).view(f"u{got.itemsize}"))
        raise AssertionError(f"{what}: {len(bad)} differ, first at {bad[:5].tolist()}: got {got.reshape(-1)[bad[:5]].tolist()} "
                             f"want {want.reshape(-1)[bad[:5]].tolist()}")


# ---- the model ---------------------------------------------------------------------------------------------------------------
def zone_of(v):
    """The zone of one label (a float32): the label when it is a whole number in [1, 2^24], else 0."""
    v = float(F32(v))
    if math.isnan(v) or math.isinf(v) or not (1.0 <= v <= float(MAX_ZONE)) or v != math.floor(v):
        return 0
    return int(v)


def zone_max(labels):
    return max([zone_of(v) for v in np.asarray(labels, F32).reshape(-1)] + [0])


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def fold(labels, Z, planes=None, cube=None):
    """-> dict(cells, n, s1, s2, counts): the 64-bit tables of zones 1..Z, a zone above Z skipped.  planes: (N, S1, S2), (h, w)
    each; cube: (bins, h, w)."""
    labels = np.asarray(labels, F32)
    h, w = labels.shape
    cells, n, s1, s2 = ([0] * Z for _ in range(4))
    bins = 0 if cube is None else cube.shape[0]
    counts = [[0] * bins for _ in range(Z)]
    for r in range(h):
        for c in range(w):
            z = zone_of(labels[r, c])
            if z == 0 or z > Z:
                continue
            cells[z - 1] = (cells[z - 1] + 1) & M64
            if planes is not None:
                n[z - 1] = (n[z - 1] + int(planes[0][r, c])) & M64
                s1[z - 1] = (s1[z - 1] + int(planes[1][r, c])) & M64
                s2[z - 1] = (s2[z - 1] + int(planes[2][r, c])) & M64
            row = counts[z - 1]
            for b in range(bins):
                v = int(cube[b, r, c])
                if v:
                    row[b] = (row[b] + v) & M64
    out = dict(cells=np.array(cells, U64))
    if planes is not None:
        out.update(n=np.array(n, U64), s1=np.array([_signed(v) for v in s1], I64), s2=np.array(s2, U64))
    if cube is not None:
        out["counts"] = np.array(counts, U64).reshape(Z, bins)
    return out


def _nan(Z):
    return np.full(Z, NAN_BITS, U32).view(F32)


def rows_stats(n, s1, s2, origin, res, ddof):
    """-> (mean, var, std) float32 columns: cs::bands_of with a 64-bit n, one rounded binary64 operation at a time."""
    Z = len(n)
    mean, var, std = _nan(Z), _nan(Z), _nan(Z)
    origin, res = float(origin), float(res)
    for k in range(Z):
        N, S1, S2 = int(n[k]), int(s1[k]), int(s2[k])
        if N == 0:
            continue
        mean[k] = F32(origin + res * (float(S1) / float(N)))
        if N <= ddof:
            continue
        d = (N * S2 - S1 * S1) % (1 << 128)
        hi, lo = d >> 64, d & M64
        dd = float(hi) * 2.0 ** 64 + float(lo)
        den = float(N) * float(N - ddof)
        vq = dd / den
        with np.errstate(all="ignore"):
            var[k] = F32((res * res) * vq)
            std[k] = F32(res * math.sqrt(vq))
    return mean, var, std


def rows_percentiles(counts, lo, w, qs):
    """-> (hist_n uint64, [column per q]): the sum of the bins, the rank, the walk, value_at."""
    counts = np.asarray(counts, U64)
    Z, bins = counts.shape
    hist_n = np.zeros(Z, U64)
    cols = [_nan(Z) for _ in qs]
    lo, w = float(lo), float(w)
    for z in range(Z):
        row = [int(v) for v in counts[z]]
        n = sum(row) & M64
        hist_n[z] = n
        if n == 0:
            continue
        for j, q in enumerate(qs):
            k = min(max(int(math.ceil(float(F32(q)) * float(n))), 1), n)
            below = 0
            for b in range(bins):
                c = row[b]
                if c != 0 and ((below + c) & M64) >= k:
                    pos = (float(k - below) - 0.5) / float(c)
                    cols[j][z] = F32(lo + w * (float(b) + pos))
                    break
                below = (below + c) & M64
    return hist_n, cols


def hist_consts(lo, hi, bins):
    """(lo, w) as the pipelines' plan computes them from a HistogramConfig's float bounds."""
    lo64 = float(F32(lo))
    return lo64, (float(F32(hi)) - lo64) / bins


def table(labels, stats=(), hists=(), Z=None):
    """The dict Pipeline.zonal returns.  stats: (channel, (N, S1, S2), origin, res, ddof); hists: (channel, cube, lo, w, qs)."""
    Z = zone_max(labels) if Z is None else Z
    out = dict(zone=np.arange(1, Z + 1, dtype=np.int32), cells=fold(labels, Z)["cells"].astype(I64))
    for ch, planes, origin, res, ddof in stats:
        f = fold(labels, Z, planes=planes)
        out[ch + "_n"] = f["n"]
        out[ch + "_mean"], out[ch + "_var"], out[ch + "_std"] = rows_stats(f["n"], f["s1"], f["s2"], origin, res, ddof)
    counts = []
    for ch, cube, lo, w, qs in hists:
        f = fold(labels, Z, cube=cube)
        counts.append(f["counts"])
        out[ch + "_hist_n"], cols = rows_percentiles(f["counts"], lo, w, qs)
        for q, col in zip(qs, cols):
            out[f"{ch}_p{int(math.floor(float(F32(q)) * 100.0 + 0.5))}"] = col
    return out, counts


def same_table(got, want, what=""):
    assert list(got.keys()) == list(want.keys()), f"{what}: columns {list(got.keys())} against {list(want.keys())}"
    for k in want:
        bits_equal(np.asarray(got[k]), np.asarray(want[k]), f"{what} column {k}")


# ---- the C-ABI: kernels (device=True) and host twins on the same arrays ---------------------------------------------------------
def strided(a, stride, offset=0, fill=0xEE):
    """(buffer, view): `a` inside a buffer of its dtype filled with bytes `fill`, rows `stride` elements apart, `offset` in."""
    a = np.ascontiguousarray(a)
    h, w = a.shape
    buf = np.empty(offset + h * stride + 7, a.dtype)
    buf.view(np.uint8)[:] = fill
    view = np.lib.stride_tricks.as_strided(buf[offset:], (h, w), (a.itemsize * stride, a.itemsize))
    view[...] = a
    return buf, view


class Mem:
    """Arrays where a run wants them: numpy copies (host twins) or device buffers (kernels)."""

    def __init__(self, A, device):
        self.A, self.device, self.keep = A, device, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.device:
            d = self.A.DeviceBuffer.from_numpy(a)
            self.keep.append(d)
            return d.ptr.value, (lambda: d.to_numpy(a.dtype, a.shape))
        c = a.copy()
        self.keep.append(c)
        return c.ctypes.data, (lambda: c)

    def call(self, name, *args):
        L = self.A.lib()
        if self.device:
            self.A.check(getattr(L, name)(*args, None))
            self.A.check(L.pcr_hip_stream_synchronize(None))
        else:
            self.A.check(getattr(L, name + "_host")(*args))

    def free(self):
        for d in self.keep:
            if self.device:
                d.free()
        self.keep = []


def guarded(Z, width=1, dtype=U64):
    """A zeroed table of Z rows of `width` words between GUARD sentinel words on either side."""
    t = np.zeros(2 * GUARD + Z * width, dtype)
    s = np.array([SENTINEL], U64).view(dtype) if np.dtype(dtype).itemsize == 8 else np.array([SENTINEL & 0xFFFFFFFF], U32).view(dtype)
    t[:GUARD] = s[0]
    t[GUARD + Z * width:] = s[0]
    return t


def unguard(t, Z, width=1, what=""):
    want = guarded(Z, width, t.dtype)
    assert np.array_equal(t[:GUARD].view(np.uint8), want[:GUARD].view(np.uint8)), f"{what}: written below the table"
    assert np.array_equal(t[GUARD + Z * width:].view(np.uint8), want[GUARD + Z * width:].view(np.uint8)), f"{what}: written above the table"
    body = t[GUARD:GUARD + Z * width].copy()
    return body.reshape(Z, width) if width > 1 else body


def run_zone_max(A, device, labels, stride=None, offset=0):
    labels = np.ascontiguousarray(labels, F32)
    h, w = labels.shape
    stride = stride or w
    m = Mem(A, device)
    buf, _ = strided(labels, stride, offset)
    p, _ = m.put(buf)
    if device:
        o, fetch = m.put(np.array([0xFFFFFFFF, SENTINEL & 0xFFFFFFFF], U32))       # (the call zeroes its word, and only that)
        m.call("pcr_hip_zone_max", p + 4 * offset, w, h, stride, o)
        got = fetch()
        assert got[1] == SENTINEL & 0xFFFFFFFF
        z = int(got[0])
    else:
        out = C.c_uint32(0xFFFFFFFF)
        m.call("pcr_hip_zone_max", p + 4 * offset, w, h, stride, C.byref(out))
        z = out.value
    m.free()
    return z


def run_fold_stats(A, device, labels, planes, Z, combine=1, stride=None, offset=0, cells=True):
    """-> dict(cells, n, s1, s2) of the entry point on strided planes and guarded tables.  planes None: cells alone."""
    labels = np.ascontiguousarray(labels, F32)
    h, w = labels.shape
    stride = stride or w
    m = Mem(A, device)
    lbuf, _ = strided(labels, stride, offset)
    lp, lfetch = m.put(lbuf)
    pp, pfetch, pbufs = [None] * 3, [], []
    if planes is not None:
        for k, (a, t) in enumerate(zip(planes, (U32, I64, U64))):
            b, _ = strided(np.ascontiguousarray(a, t), stride, offset)
            p, f = m.put(b)
            pp[k] = p + b.itemsize * offset
            pfetch.append(f)
            pbufs.append(b)
    tabs = {}
    for name, t, on in (("cells", U64, cells), ("n", U64, planes is not None), ("s1", I64, planes is not None), ("s2", U64, planes is not None)):
        tabs[name] = m.put(guarded(Z, 1, t)) if on else (None, None)
    at = lambda name: tabs[name][0] + 8 * GUARD if tabs[name][0] else None
    prm = A.ZoneFoldParams(combine)
    m.call("pcr_hip_zone_fold_stats", lp + 4 * offset, w, h, stride, pp[0], pp[1], pp[2], stride, Z, C.byref(prm), at("cells"), at("n"),
           at("s1"), at("s2"))
    assert np.array_equal(lfetch().view(U32), lbuf.view(U32)), "the label band is only read"
    for f, b in zip(pfetch, pbufs):
        assert np.array_equal(f().view(np.uint8), b.view(np.uint8)), "a plane is only read"
    out = {name: unguard(f(), Z, 1, name) for name, (p, f) in tabs.items() if p}
    m.free()
    return out


def run_fold_hist(A, device, labels, cube, Z, combine=1, stride=None, offset=0, gap=0):
    """-> counts (Z, bins) uint64.  The cube's planes are `gap` elements further apart than they need be."""
    labels = np.ascontiguousarray(labels, F32)
    cube = np.ascontiguousarray(cube, U32)
    bins, h, w = cube.shape
    stride = stride or w
    m = Mem(A, device)
    lbuf, _ = strided(labels, stride, offset)
    lp, _ = m.put(lbuf)
    plane = (h - 1) * stride + w + gap
    cbuf = np.empty(offset + bins * plane + 7, U32)
    cbuf.view(np.uint8)[:] = 0xEE
    for b in range(bins):
        np.lib.stride_tricks.as_strided(cbuf[offset + b * plane:], (h, w), (4 * stride, 4))[...] = cube[b]
    cp, cfetch = m.put(cbuf)
    tp, tfetch = m.put(guarded(Z, bins))
    prm = A.ZoneFoldParams(combine)
    m.call("pcr_hip_zone_fold_hist", lp + 4 * offset, w, h, stride, cp + 4 * offset, bins, stride, plane, Z, C.byref(prm), tp + 8 * GUARD)
    assert np.array_equal(cfetch(), cbuf), "the cube is only read"
    out = unguard(tfetch(), Z, bins, "counts").reshape(Z, bins)
    m.free()
    return out


def run_rows_stats(A, device, n, s1, s2, origin, res, ddof):
    Z = len(n)
    m = Mem(A, device)
    ins = [m.put(np.ascontiguousarray(a, t))[0] for a, t in ((n, U64), (s1, I64), (s2, U64))]
    outs = [m.put(guarded(Z, 1, F32)) for _ in range(3)]
    m.call("pcr_hip_zone_rows_stats", *ins, Z, float(origin), float(res), ddof, *[p + 4 * GUARD for p, _ in outs])
    cols = tuple(unguard(f(), Z, 1, "rows") for _, f in outs)
    m.free()
    return cols


def run_rows_percentiles(A, device, counts, lo, w, qs):
    counts = np.ascontiguousarray(counts, U64)
    Z, bins = counts.shape
    m = Mem(A, device)
    cp, _ = m.put(counts)
    np_, nfetch = m.put(guarded(Z))
    outs = [m.put(guarded(Z, 1, F32)) for _ in qs]
    q = np.array(qs, F32)
    ptrs = (C.c_void_p * max(len(qs), 1))(*[p + 4 * GUARD for p, _ in outs])
    m.call("pcr_hip_zone_rows_percentiles", cp, bins, Z, float(lo), float(w), len(qs), q.ctypes.data if len(qs) else None,
           np_ + 8 * GUARD, ptrs if len(qs) else None)
    hist_n = unguard(nfetch(), Z, 1, "hist_n")
    cols = [unguard(f(), Z, 1, "percentile") for _, f in outs]
    m.free()
    return hist_n, cols


# ---- what the tests fold --------------------------------------------------------------------------------------------------------
# (2^24 + 1 is no Float32 -- it rounds to 2^24, a zone: the first label above the range that a band can hold is 2^24 + 2)
INVALID = [float("nan"), float("inf"), -float("inf"), 0.0, -3.0, 2.5, -0.0, float(MAX_ZONE + 2)]


def random_planes(h, w, seed):
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 40, (h, w)).astype(U32)
    s1 = rng.integers(-(1 << 30), 1 << 30, (h, w)).astype(I64)
    s2 = rng.integers(0, 1 << 50, (h, w)).astype(U64)
    n[rng.random((h, w)) < 0.2] = 0
    return n, s1, s2


def random_cube(bins, h, w, seed):
    rng = np.random.default_rng(seed)
    cube = rng.integers(0, 9, (bins, h, w)).astype(U32)
    cube[rng.random((bins, h, w)) < 0.6] = 0
    return cube


def label_patterns(h, w, seed=3):
    """name -> (labels, Z passed to the folds): the ways equal labels can lie in a wave of 64 consecutive cells."""
    rng = np.random.default_rng(seed)
    cells = h * w
    flat = lambda a: np.asarray(a, F32).reshape(h, w)
    out = {}
    out["one zone"] = (flat(np.full(cells, 5.0)), 5)
    out["all distinct"] = (flat(np.arange(1, cells + 1)), cells)
    out["alternating"] = (flat(1 + (np.arange(cells) % 2)), 2)
    for run in (63, 64, 65):
        out[f"runs of {run}"] = (flat(1 + (np.arange(cells) // run) % 7), 7)
    gap = np.full(cells, 3.0)
    gap[64:128] = np.nan                                         # a whole wave with no zone (where the band has a second wave)
    gap[:5] = 0.0
    out["a wave with no zone"] = (flat(gap), 3)
    mixed = 1 + (np.arange(cells) // 9) % 11
    mixed = mixed.astype(F64)
    at = rng.choice(cells, size=max(cells // 5, min(cells, len(INVALID))), replace=False)
    mixed[at] = np.resize(np.array(INVALID), len(at))
    out["invalid labels scattered in"] = (flat(mixed), 11)
    above = 1 + (np.arange(cells) // 5) % 9
    out["labels above Z"] = (flat(above), 4)                     # zones 5..9 must be ignored
    top = 1 + (np.arange(cells) % 3).astype(F64)
    top[cells // 2] = float(MAX_ZONE)
    out["2^24"] = (flat(top), 3)                                 # (a valid zone, above the Z passed in)
    return out


def carry_planes():
    """Labels and planes whose zone sums carry: zone 1's n passes 2^32 and its s2 2^63 (and wraps 2^64), its s1 changes sign;
    zone 2 has n = 1 (ddof 1: no spread); zone 3 has cells with no point; zone 4 has no cell."""
    labels = np.array([[1, 1, 1, 1, 2, 3, 3, 5, 1, 1]], F32)
    n = np.array([[2 ** 32 - 1] * 4 + [1, 0, 0, 7, 2 ** 32 - 1, 5]], U32)
    s1 = np.array([[1 << 40, -(1 << 41), 1 << 39, -(1 << 62), 77, 0, 0, -21, 1 << 62, 3]], I64)
    s2 = np.array([[(1 << 62) + 5, (1 << 62) + 7, (1 << 63) + 11, (1 << 63) + 13, 77 * 77, 0, 0, 63, 1 << 50, 9]], U64)
    return labels, (n, s1, s2), 5


def carry_cube(bins):
    """One zone over four cells whose bin counts sum past 2^32 in the bin the upper ranks land on."""
    labels = np.array([[1, 1, 1, 1, 2, 0]], F32)
    cube = np.zeros((bins, 1, 6), U32)
    cube[0, 0, :4] = [3, 0, 1, 0]
    cube[bins - 1, 0, :4] = 2 ** 32 - 1
    if bins > 2:
        cube[bins // 2, 0, :4] = [2 ** 31, 2 ** 31, 5, 0]
    cube[0, 0, 4] = 1
    return labels, cube, 2


# ---- the pipelines' common ground -------------------------------------------------------------------------------------------------
STAT = dict(origin=0.0, res=0.01, ddof=1)                    # the cell-stats entry of pipeline_cfg
HIST = dict(lo=0.0, hi=32.0, bins=32, qs=[0.5, 0.95])        # ... and its histogram


def cones():
    """The two cones of the trees' known answer: crowns of 97 and 37 cells on a 40 x 32 grid."""
    rr, cc = np.mgrid[0:32, 0:40]
    return np.maximum(np.maximum(0.0, 20.0 - 2.0 * np.hypot(rr - 10, cc - 10)), np.maximum(0.0, 12.0 - 2.0 * np.hypot(rr - 10, cc - 24))).astype(F32)


def pipeline_cfg(pcr, W, H, mode, location=None):
    """Min, Max and Count of `value`, the trees of the Max band, one cell-stats entry and one histogram of `value`, and the table
    of both by tree."""
    import ground_filter_common as G
    import trees_common as T
    cfg = G.pipeline_cfg(W, H, mode, ground=False)
    if location is not None:
        cfg.result_location = location
    cfg.trees = [T.band_cfg("value_1")]
    cfg.cell_stats = [pcr.CellStatsConfig("value", STAT["origin"], STAT["res"], [pcr.CellStat.Mean], STAT["ddof"])]
    cfg.histograms = [pcr.HistogramConfig("value", HIST["lo"], HIST["hi"], HIST["bins"], HIST["qs"])]
    cfg.zonal = [pcr.ZonalConfig("value_1_tree_id", cell_stats=[0], histograms=[0])]
    return cfg


def create(pcr, cfg, engine):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == engine
    return pipe


def cloud_of_band(pcr, z):
    """One point per finite cell of z at its centre, the value as the channel `value`."""
    h, w = z.shape
    rr, cc = np.nonzero(np.isfinite(z))
    return _cloud(pcr, cc + 0.5, h - (rr + 0.5), z[rr, cc])


def _cloud(pcr, x, y, v):
    c = pcr.PointCloud.create(len(x))
    c.set_x_array(np.ascontiguousarray(x, F64))
    c.set_y_array(np.ascontiguousarray(y, F64))
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", np.ascontiguousarray(v, F32))
    return c


CLOUDS = {}


def canopy_points(pcr, W, H, seed, extra=5000):
    """A canopy's top return in every cell with data and `extra` lower returns scattered under it: a few thousand points whose
    Max band is the canopy and whose cells hold one to several points."""
    import trees_common as T
    if (W, H, seed) not in CLOUDS:
        z = T.canopy(W, H, seed)
        z[~np.isfinite(z)] = np.nan
        z[z <= 0.0] = 0.0
        rng = np.random.default_rng(100 + seed)
        rr, cc = np.nonzero(~np.isnan(z))
        er, ec = rng.integers(0, H, extra), rng.integers(0, W, extra)
        ok = ~np.isnan(z[er, ec])
        er, ec = er[ok], ec[ok]
        x = np.concatenate([cc + 0.5, ec + rng.uniform(0.05, 0.95, len(ec))])
        y = np.concatenate([H - (rr + 0.5), H - (er + rng.uniform(0.05, 0.95, len(er)))])
        v = np.concatenate([z[rr, cc], z[er, ec] * rng.uniform(0.1, 1.0, len(er)).astype(F32)])
        CLOUDS[(W, H, seed)] = (x, y, v.astype(F32))
    return _cloud(pcr, *CLOUDS[(W, H, seed)])


def plot_labels(W, H, plot=16):
    """Square plots of `plot` cells numbered row-major from 1, a strip with no plot and a few labels that are none."""
    rr, cc = np.mgrid[0:H, 0:W]
    lab = (1 + (rr // plot) * ((W + plot - 1) // plot) + cc // plot).astype(F32)
    lab[:, W // 2] = np.nan
    lab[0, :8] = INVALID
    return lab


def pipeline_model(pcr, pipe, labels=None, qs=None):
    """The model applied to the pipeline's own state: pipe.cell_stats(0), pipe.histogram(0) and the tree_id band (or `labels`)."""
    import histogram_common as H
    if labels is None:
        names, bands = H.result_bands(pipe)
        labels = bands[names.index("value_1_tree_id")]
    lo, w = hist_consts(HIST["lo"], HIST["hi"], HIST["bins"])
    return table(labels, stats=[("value", pipe.cell_stats(0), STAT["origin"], STAT["res"], STAT["ddof"])],
                 hists=[("value", pipe.histogram(0), lo, w, HIST["qs"] if qs is None else qs)])
