"""Shared by tests/test_point_zonal.py and tests/test_gpu_point_zonal.py: the model of the point-zonal contract (include/pcr_hip.h,
"point zonal tables"; csrc/point_zonal.hpp) -- no engine code: plain loops over Python ints, zone_of, step_of and bin_of point by
point, every counter reduced modulo 2^64 -- and ctypes drivers of the C-ABI's kernels and host twins on inputs that can start one
element, or one byte, off a 16-byte boundary and on tables between sentinel words.  Every comparison made with it is on the
bits; the rows are zonal_common's."""
import ctypes as C
import math

import numpy as np

import zonal_common as ZC
from zonal_common import GUARD, M64, MAX_ZONE, SENTINEL, bits_equal, guarded, unguard, zone_of

F32, F64 = np.float32, np.float64
U8, U32, I64, U64 = np.uint8, np.uint32, np.int64, np.uint64
Q = 1 << 21                                  # cs::kQ: |step| <= Q
SEED = (1 << 64) - 3                         # what a table holds beforehand where a sum shall wrap


# ---- the model ---------------------------------------------------------------------------------------------------------------
def step_of(v, origin, inv_res):
    """cs::step_of: None for NaN; ((double)v - origin) * inv_res clamped to +-2^21, else rounded to nearest, ties to even."""
    v = float(F32(v))
    if math.isnan(v):
        return None
    t = (v - float(origin)) * float(inv_res)
    if t <= -float(Q):
        return -Q
    if t >= float(Q):
        return Q
    return int(round(t))                     # (Python rounds a float half to even)


def bin_of(v, lo, inv_w, bins):
    """hist::bin_of: None for NaN; below the range bin 0, at or above it the last bin."""
    v = float(F32(v))
    if math.isnan(v):
        return None
    t = (v - float(lo)) * float(inv_w)
    if t < 0.0:
        return 0
    if t >= float(bins):
        return bins - 1
    return int(t)


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def fold(labels, mask, values, Z, stat=None, hist=None, seed=0, info=(0, 0)):
    """-> dict(points, info[, n, s1, s2][, counts]): tables of capacity Z that held `seed` in every word, info words that held
    `info`.  stat: (origin, inv_res); hist: (bins, lo, inv_w); mask None: every point kept."""
    labels = np.asarray(labels, F32).reshape(-1)
    points, n, s1, s2 = ([seed] * Z for _ in range(4))
    bins = hist[0] if hist else 0
    counts = [[seed] * bins for _ in range(Z)]
    zmax, over = int(info[0]), int(info[1])
    for i in range(len(labels)):
        if mask is not None and int(mask[i]) == 0:
            continue
        z = zone_of(labels[i])
        if z == 0:
            continue
        if z > Z:
            over = (over + 1) & M64
            continue
        zmax = max(zmax, z)
        points[z - 1] = (points[z - 1] + 1) & M64
        if stat:
            q = step_of(values[i], *stat)
            if q is not None:
                n[z - 1] = (n[z - 1] + 1) & M64
                s1[z - 1] = (s1[z - 1] + q) & M64
                s2[z - 1] = (s2[z - 1] + q * q) & M64
        if hist:
            b = bin_of(values[i], hist[1], hist[2], bins)
            if b is not None:
                counts[z - 1][b] = (counts[z - 1][b] + 1) & M64
    out = dict(points=np.array(points, U64), info=np.array([zmax, over], U64))
    if stat:
        out.update(n=np.array(n, U64), s1=np.array([_signed(v) for v in s1], I64), s2=np.array(s2, U64))
    if hist:
        out["counts"] = np.array(counts, U64).reshape(Z, bins)
    return out


def column_name(ch, q):
    return f"{ch}_p{int(math.floor(float(F32(q)) * 100.0 + 0.5))}"


def table(labels, Z, stats=(), hists=()):
    """The dict Pipeline.point_zonal returns, and the histograms' counts.  stats: (channel, values, mask, origin, res, ddof);
    hists: (channel, values, mask, lo, hi, bins, qs); `points` counts the points of points_mask.  Rows up to the greatest zone
    any point of any mask carried."""
    return _table(labels, Z, stats, hists)


def _table(labels, Z, stats, hists, points_mask=None):
    base = fold(labels, points_mask, None, Z)
    top = int(base["info"][0])
    folds_s = [fold(labels, m, v, Z, stat=(o, 1.0 / r)) for _, v, m, o, r, _ in stats]
    folds_h = []
    for _, v, m, lo, hi, bins, _ in hists:
        lo64, w = ZC.hist_consts(lo, hi, bins)
        folds_h.append(fold(labels, m, v, Z, hist=(bins, lo64, float(bins) / (float(F32(hi)) - lo64))))
    out = dict(zone=np.arange(1, top + 1, dtype=np.int32), points=base["points"][:top].astype(I64))
    for (ch, _, _, o, r, ddof), f in zip(stats, folds_s):
        out[ch + "_n"] = f["n"][:top]
        out[ch + "_mean"], out[ch + "_var"], out[ch + "_std"] = ZC.rows_stats(f["n"][:top], f["s1"][:top], f["s2"][:top], o, r, ddof)
    counts = []
    for (ch, _, _, lo, hi, bins, qs), f in zip(hists, folds_h):
        lo64, w = ZC.hist_consts(lo, hi, bins)
        counts.append(f["counts"][:top])
        out[ch + "_hist_n"], cols = ZC.rows_percentiles(f["counts"][:top], lo64, w, qs)
        for q, col in zip(qs, cols):
            out[column_name(ch, q)] = col
    return out, counts


def table_masked(labels, Z, points_mask, stats=(), hists=()):
    return _table(labels, Z, stats, hists, points_mask)


# ---- the C-ABI: kernels (device=True) and host twins on the same arrays ---------------------------------------------------------
class Placed:
    """`a` in memory `off` BYTES past a 16-byte boundary (device or host), between filler bytes that must stay as they are."""

    def __init__(self, m, a, off):
        a = np.ascontiguousarray(a)
        self.a, self.m = a, m
        raw = np.full(a.nbytes + 64, 0xEE, U8)
        host_pad = 0 if m.device else (-raw.ctypes.data) % 16
        self.start = 16 + host_pad + off
        raw[self.start:self.start + a.nbytes] = a.view(U8).reshape(-1)
        if m.device:
            base, self.fetch = m.put(raw)
        else:                                                    # (in place: a copy would move the boundary)
            m.keep.append(raw)
            base, self.fetch = raw.ctypes.data, (lambda: raw)
        self.ptr = base + self.start
        assert self.ptr % 16 == off % 16

    def unchanged(self, what):
        assert np.array_equal(np.asarray(self.fetch()).view(U8).reshape(-1), self.raw_before()), f"{what} is only read"

    def raw_before(self):
        raw = np.full(self.a.nbytes + 64, 0xEE, U8)
        raw[self.start:self.start + self.a.nbytes] = self.a.view(U8).reshape(-1)
        return raw


def _tables(m, names, Z, width, seed):
    tabs = {}
    for name, t, on in names:
        if not on:
            tabs[name] = (None, None)
            continue
        g = guarded(Z, width if name == "counts" else 1, t)
        body = g[GUARD:len(g) - GUARD].view(U64)
        body[:] = seed
        tabs[name] = m.put(g)
    return tabs


def _info(m, info):
    """The two info words between sentinels."""
    g = guarded(2)
    g[GUARD:GUARD + 2] = np.array(info, U64)
    return m.put(g)


def run_fold_stats(A, device, labels, mask, values, Z, origin=0.0, inv_res=100.0, path=0, blocks=0, points=True, seed=0, info=(0, 0),
                   off=(0, 0, 0), calls=1):
    """-> dict(points, n, s1, s2, info) of pcr_hip_point_fold_stats[_host].  values None: `points` alone; info None: no info
    words; off: the byte offsets of label, mask and value from a 16-byte boundary; calls: the cloud in that many consecutive
    pieces, one call each, into the same tables."""
    labels = np.ascontiguousarray(labels, F32).reshape(-1)
    n = len(labels)
    m = ZC.Mem(A, device)
    lab = Placed(m, labels, off[0])
    msk = Placed(m, np.ascontiguousarray(mask, U8), off[1]) if mask is not None else None
    val = Placed(m, np.ascontiguousarray(values, F32), off[2]) if values is not None else None
    has = values is not None
    tabs = _tables(m, (("points", U64, points), ("n", U64, has), ("s1", I64, has), ("s2", U64, has)), Z, 1, seed)
    at = lambda name: tabs[name][0] + 8 * GUARD if tabs[name][0] else None
    ip, ifetch = _info(m, info) if info is not None else (None, None)
    prm = A.PointFoldParams(path, blocks)
    edges = [n * k // calls for k in range(calls + 1)]
    for a, b in zip(edges[:-1], edges[1:]):
        m.call("pcr_hip_point_fold_stats", lab.ptr + 4 * a, msk.ptr + a if msk else None, val.ptr + 4 * a if val else None, b - a,
               float(origin), float(inv_res), Z, C.byref(prm), at("points"), at("n"), at("s1"), at("s2"), ip + 8 * GUARD if ip else None)
    for x, what in ((lab, "the label"), (msk, "the mask"), (val, "the value")):
        if x is not None:
            x.unchanged(what)
    out = {name: unguard(f(), Z, 1, name) for name, (p, f) in tabs.items() if p}
    if ip:
        out["info"] = unguard(ifetch(), 2, 1, "info")
    m.free()
    return out


def run_fold_hist(A, device, labels, mask, values, Z, bins, lo=0.0, inv_w=1.0, path=0, blocks=0, seed=0, info=(0, 0), off=(0, 0, 0),
                  calls=1):
    """-> dict(counts (Z, bins), info) of pcr_hip_point_fold_hist[_host]."""
    labels = np.ascontiguousarray(labels, F32).reshape(-1)
    n = len(labels)
    m = ZC.Mem(A, device)
    lab = Placed(m, labels, off[0])
    msk = Placed(m, np.ascontiguousarray(mask, U8), off[1]) if mask is not None else None
    val = Placed(m, np.ascontiguousarray(values, F32), off[2])
    tabs = _tables(m, (("counts", U64, True),), Z, bins, seed)
    ip, ifetch = _info(m, info) if info is not None else (None, None)
    prm = A.PointFoldParams(path, blocks)
    edges = [n * k // calls for k in range(calls + 1)]
    for a, b in zip(edges[:-1], edges[1:]):
        m.call("pcr_hip_point_fold_hist", lab.ptr + 4 * a, msk.ptr + a if msk else None, val.ptr + 4 * a, b - a, bins, float(lo),
               float(inv_w), Z, C.byref(prm), tabs["counts"][0] + 8 * GUARD, ip + 8 * GUARD if ip else None)
    for x, what in ((lab, "the label"), (msk, "the mask"), (val, "the value")):
        if x is not None:
            x.unchanged(what)
    out = dict(counts=unguard(tabs["counts"][1](), Z, bins, "counts").reshape(Z, bins))
    if ip:
        out["info"] = unguard(ifetch(), 2, 1, "info")
    m.free()
    return out


def same(got, want, what=""):
    assert sorted(got) == sorted(want), f"{what}: {sorted(got)} against {sorted(want)}"
    for k in want:
        bits_equal(np.asarray(got[k]), np.asarray(want[k]), f"{what}: {k}")


# ---- what the tests fold --------------------------------------------------------------------------------------------------------
INVALID = [0.0, -0.0, -1.0, 2.5, float("nan"), float("inf"), -float("inf"), float(MAX_ZONE + 2)]


def label_patterns(n, Z, seed=5):
    """name -> labels (n of them) for a table of capacity Z >= 7: the ways equal labels can lie in a wave."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    out = {}
    out["one zone"] = np.full(n, 5.0)
    out["alternating"] = 1.0 + (i % 2)
    for run in (1, 63, 64, 65, 200):
        out[f"runs of {run}"] = 1.0 + (i // run) % 7
    edge = 1.0 + (i // 9) % 7
    at = rng.choice(n, size=min(n, max(n // 4, 12)), replace=False)
    edge[at] = np.resize(np.array(INVALID + [float(Z), float(Z + 1), float(MAX_ZONE), 1.0, 3.0]), len(at))
    out["edge labels scattered in"] = edge
    shuffled = 1.0 + (3 * i + i // 7) % 7                        # no two neighbours equal: they differ by 3 or 4 modulo 7
    out["shuffled"] = shuffled
    return {k: np.asarray(v, F32) for k, v in out.items()}


def values_for(n, seed=9, origin=0.0, inv_res=100.0):
    """Values with the edge cases scattered in: NaN, +-Inf, exactly at the +-2^21 step clamp and one step inside it, negatives."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-40.0, 70.0, n)
    res = 1.0 / inv_res
    edges = [float("nan"), float("inf"), -float("inf"), origin + Q * res, origin - Q * res, origin + (Q - 1) * res,
             origin - (Q - 1) * res, -0.0, origin + 0.5 * res, origin + 1.5 * res, origin - 2.5 * res]
    at = rng.choice(n, size=min(n, max(n // 6, len(edges))), replace=False)
    v[at] = np.resize(np.array(edges), len(at))
    return v.astype(F32)


def masks_for(n, seed=11):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 255], U8), size=n)


# ---- the pipelines' common ground -------------------------------------------------------------------------------------------------
# (the pipeline grid and the dyadic points of sample_grid_common; the plots of points_in_polygons_common, 14 of them)
STAT = dict(origin=0.0, res=0.125, ddof=1)
HIST = dict(lo=0.0, hi=64.0, bins=16, qs=[0.5, 0.95])
CFG_FILT = [("cls", "NotEqual", 5.0)]        # PipelineConfig::filter
STAT_FILT = [("ret", "Equal", 1.0)]          # the stats spec's own
HIST_FILT = [("z", "Less", 40.0)]            # the histogram's own


def entry(pcr, label="plot", max_zones=64, stat_filt=(), hist_filt=(), stat=True, hist=True):
    import reduction_filters_common as RF
    cs = pcr.CellStatsConfig("z", STAT["origin"], STAT["res"], [pcr.CellStat.StdDev], STAT["ddof"])
    h = pcr.HistogramConfig("z", HIST["lo"], HIST["hi"], HIST["bins"], HIST["qs"])
    cs.filter = RF.filter_spec(stat_filt)
    h.filter = RF.filter_spec(hist_filt)
    return pcr.PointZonalConfig(label, [cs] if stat else [], [h] if hist else [], max_zones)


def keeps(c, preds):
    """The byte mask of a conjunction of (channel, op, value) predicates over a cloud dict."""
    ops = dict(Equal=np.equal, NotEqual=np.not_equal, Less=np.less, LessEqual=np.less_equal, Greater=np.greater,
               GreaterEqual=np.greater_equal)
    m = np.ones(len(c["x"]), bool)
    for ch, op, v in preds:
        m &= ops[op](np.asarray(c[ch], F32), F32(v))
    return m.astype(U8)


def pipeline_model(c, labels, Z=64, cfg_filt=(), stat_filt=(), hist_filt=()):
    """The model's table of `entry` for the cloud dict c and its labels."""
    base = keeps(c, cfg_filt)
    return table_masked(labels, Z, base,
                        stats=[("z", c["z"], base & keeps(c, stat_filt), STAT["origin"], STAT["res"], STAT["ddof"])],
                        hists=[("z", c["z"], base & keeps(c, hist_filt), HIST["lo"], HIST["hi"], HIST["bins"], HIST["qs"])])


def piece(c, a, b):
    return {k: v[a:b] for k, v in c.items()}


def plot_pipeline(pcr, mode, cfg_filt=(), **kw):
    """A pipeline on the pipeline grid with the polygon channel `plot` and one point-zonal entry by it (kw: entry's)."""
    import reduction_filters_common as RF
    import sample_grid_common as SG
    cfg = RF.make_config(mode, [RF.S("Count", ch="z")], cfg_filt, SG.PGRID, polygon_channels=[pcr.PolygonChannelConfig("plot")],
                         point_zonal=[entry(pcr, **kw)])
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == ("host" if mode == "cpu" else "hip")
    return p


def triangle_case():
    """One triangular plot on a 10 m grid of 10 x 10 cells and the points of a 1 m lattice shifted off every cell centre (5, 15,
    ...) and every cell edge (0, 10, ...): -> (grid dict, Polys, cloud dict)."""
    import rasterize_common as RC
    g = dict(min_x=0.0, min_y=0.0, max_x=100.0, max_y=100.0, cs=10.0, W=10, H=10, tw=16, th=16)
    polys = RC.Polys([[np.array([[12.3, 8.1], [87.6, 21.4], [33.3, 91.7]])]])
    jj, ii = np.mgrid[0:100, 0:100]
    x, y = (ii.ravel() + 0.37).astype(F64), (jj.ravel() + 0.41).astype(F64)
    z = ((ii.ravel() * 7 + jj.ravel() * 3) % 40 / 8.0).astype(F32)
    return g, polys, dict(x=x, y=y, z=z)
