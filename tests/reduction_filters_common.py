"""What the ReductionSpec.filter tests share: clouds, a NumPy model of the contract, and the checks that run on either engine.

The contract (pcr/engine/pipeline.h): a point contributes to a spec when it is inside the bounds, passes
PipelineConfig.filter and passes the spec's own filter; ONE touched-tile set, from PipelineConfig.filter's survivors alone;
finalize as always (Sum as is, Count / Average NaN where the count is 0, Max / Min NaN at the identity, every cell of an
untouched tile NaN).  Values are multiples of 1/8 and small integers, per-cell sums far below 2^23 units: every float32 sum is
exact in any order, so every comparison is view(uint32) equality.  No engine code is used by the model."""
import os

import numpy as np

import pcr
import pcr_oracle_py as O
from most_recent_common import assert_bits, band_of_words, fold_words
from sequence_fuzz_common import cells_of, keep_mask

FLT_MAX = np.float32(3.4028234663852886e38)
GRID = dict(min_x=0.0, min_y=0.0, max_x=40.0, max_y=24.0, cs=1.0, W=40, H=24, tw=16, th=16)      # six tiles, some partial
ONE_TILE = dict(min_x=0.0, min_y=0.0, max_x=40.0, max_y=24.0, cs=1.0, W=40, H=24, tw=64, th=64)
SIZES = (1, 63, 64, 65, 1027, 20000)           # the last one reaches the binned path
OPS = ("Equal", "NotEqual", "Less", "LessEqual", "Greater", "GreaterEqual", "InSet", "NotInSet")
CHANNELS = ("a", "t", "cls", "ret", "q")


def tiles_of(g):
    return -(-g["W"] // g["tw"]), -(-g["H"] // g["th"])


def make_points(n, seed, g=GRID, clustered=True):
    """x, y with points on the bounds, on cell edges and outside; `a` multiples of 1/8; `t` small integers; `cls` clustered by
    reference tile -- tile (0, 0) holds class 2 only, tile (0, 1) class 5 only, the others a mix of 1, 2, 5, 6; tile (1, 2)
    holds no point at all; `ret` 1..3; `q` like cls with NaNs."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, g["max_x"] + 2.0, n)
    y = rng.uniform(-2.0, g["max_y"] + 2.0, n)
    k = max(n // 8, 1)
    x[:k] = np.round(x[:k])                                      # on cell edges
    y[k:2 * k] = np.round(y[k:2 * k])
    x[2 * k:2 * k + k // 2] = rng.choice([g["min_x"], g["max_x"]], len(x[2 * k:2 * k + k // 2]))    # on the bounds
    y[2 * k + k // 2:3 * k] = rng.choice([g["min_y"], g["max_y"]], len(y[2 * k + k // 2:3 * k]))
    if clustered:
        empty = (x >= 32.0) & (y <= 8.0)                         # tile (1, 2): cols 32.., rows 16..
        x[empty] -= 16.0
    cls = rng.choice(np.array([1, 2, 5, 6], np.float32), n)
    if clustered:
        cell = cells_of(g, x, y)
        tr, tc = (cell // g["W"]) // g["th"], (cell % g["W"]) // g["tw"]
        cls[(cell >= 0) & (tr == 0) & (tc == 0)] = 2.0
        cls[(cell >= 0) & (tr == 0) & (tc == 1)] = 5.0
    q = cls.copy()
    q[rng.random(n) < 0.2] = np.nan
    return dict(x=x, y=y, a=(rng.integers(-64, 65, n) / 8.0).astype(np.float32), t=rng.integers(0, 6, n).astype(np.float32),
                cls=cls.astype(np.float32), ret=rng.integers(1, 4, n).astype(np.float32), q=q.astype(np.float32))


# ---- predicates: (channel, op name, value or list of values) ---------------------------------------------------------------------
def pred_mask(c, pred):
    ch, op, v = pred
    with np.errstate(invalid="ignore"):
        return keep_mask(dict(op=op, value=0.0 if isinstance(v, (list, tuple)) else v, set=list(v) if isinstance(v, (list, tuple)) else []),
                         c[ch])


def conj_mask(c, preds):
    keep = np.ones(len(c["x"]), bool)
    for p in preds:
        keep &= pred_mask(c, p)
    return keep


def filter_spec(preds, into=None):
    f = into if into is not None else pcr.FilterSpec()
    for ch, op, v in preds:
        if op == "InSet":
            f.add_in_set(ch, [float(s) for s in v])
        elif op == "NotInSet":
            p = pcr.FilterPredicate()
            p.channel_name, p.op, p.value_set = ch, pcr.CompareOp.NotInSet, [float(s) for s in v]
            f.predicates = list(f.predicates) + [p]
        else:
            f.add(ch, getattr(pcr.CompareOp, op), float(v))
    return f


# ---- specs: dict(type, ch, filt=[preds], ts=timestamp channel, glyph=None | dict(kind="line" | "gauss", ...)) -------------------
def S(rtype, ch="a", filt=(), ts="t", glyph=None):
    return dict(type=rtype, ch=ch, filt=list(filt), ts=ts, glyph=glyph)


def to_spec(s):
    if s["glyph"] is None:
        r = pcr.ReductionSpec()
        r.value_channel = s["ch"]
    elif s["glyph"]["kind"] == "line":
        r = pcr.line_splat_spec(s["ch"], direction_channel="dir", default_half_length=s["glyph"]["hl"], max_radius_cells=s["glyph"]["maxr"])
    else:
        r = pcr.gaussian_splat_spec(s["ch"], default_sigma=s["glyph"]["sigma"], max_radius_cells=s["glyph"]["maxr"])
    r.type = getattr(pcr.ReductionType, s["type"])
    if s["type"] == "MostRecent":
        r.timestamp_channel = s["ts"]
    filter_spec(s["filt"], into=r.filter)                        # in place: r.filter is the spec's own FilterSpec
    assert len(r.filter.predicates) == len(s["filt"])
    return r


def make_config(mode, specs, cfg_filt=(), g=GRID, **kw):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(g["min_x"], g["min_y"], g["max_x"], g["max_y"])
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = g["cs"], -g["cs"]
    cfg.grid.tile_width, cfg.grid.tile_height = g["tw"], g["th"]
    cfg.grid.compute_dimensions()
    cfg.exec_mode = pcr.ExecutionMode.CPU if mode == "cpu" else pcr.ExecutionMode.GPU
    cfg.reductions = [to_spec(s) for s in specs]
    if cfg_filt:
        cfg.filter = filter_spec(cfg_filt)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create(mode, specs, cfg_filt=(), g=GRID, **kw):
    p = pcr.Pipeline.create(make_config(mode, specs, cfg_filt, g, **kw))
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == ("host" if mode == "cpu" else "hip")
    return p


def make_cloud(c, mode, names=None):
    cloud = pcr.PointCloud.create(len(c["x"]))
    cloud.set_x_array(np.asarray(c["x"], np.float64))
    cloud.set_y_array(np.asarray(c["y"], np.float64))
    for name in names if names is not None else [k for k in c if k not in ("x", "y")]:
        cloud.add_channel(name, pcr.DataType.Float32)
        cloud.set_channel_array_f32(name, np.asarray(c[name], np.float32))
    return cloud.to_device() if mode == "gpu" else cloud


def bands(p):
    res = p.result()
    return [np.array(res.band_array(b)) for b in range(res.num_bands())]


def read_touched(p):
    """The touched flags of an in-core HIP pipeline, through the read-only pointer."""
    from conftest import load_cabi
    A = load_cabi()
    p.synchronize()
    ptr, tx, ty = p.tile_touched_ptr(readonly=True)
    out = np.empty((ty, tx), np.uint32)
    A.check(A.lib().pcr_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None))
    A.check(A.lib().pcr_hip_stream_synchronize(None))
    return out != 0


# ---- the model -------------------------------------------------------------------------------------------------------------------
class Model:
    """Per spec four float32 planes (sum, count, max, min) or a MostRecent word plane; one touched set; survivors and
    collections as stats() counts them."""
    IDENTITY = (np.float32(0.0), np.float32(0.0), -FLT_MAX, FLT_MAX)

    def __init__(self, specs, cfg_filt=(), g=GRID):
        self.g, self.specs, self.cfg_filt = g, specs, list(cfg_filt)
        self.W, self.H = g["W"], g["H"]
        tx, ty = tiles_of(g)
        self.touched = np.zeros((ty, tx), bool)
        self.survivors = self.collections = 0
        self.planes = [np.zeros(self.W * self.H, np.uint64) if s["type"] == "MostRecent"
                       else [np.full(self.W * self.H, self.IDENTITY[p], np.float32) for p in range(4)] for s in specs]

    def ingest(self, c):
        keep0 = conj_mask(c, self.cfg_filt)
        if not keep0.any():
            return                                               # not a collection
        self.survivors += int(keep0.sum())
        self.collections += 1
        cell = cells_of(self.g, c["x"], c["y"])
        ok0 = keep0 & (cell >= 0)
        self.touched[(cell[ok0] // self.W) // self.g["th"], (cell[ok0] % self.W) // self.g["tw"]] = True
        for s, pl in zip(self.specs, self.planes):
            keep = keep0 & conj_mask(c, s["filt"])               # the conjunction of the two predicate lists
            ok = keep & (cell >= 0)
            v = c[s["ch"]]
            if s["type"] == "MostRecent":
                fold_words(cell, v, c[s["ts"]], self.W * self.H, keep=keep, words=pl)
                continue
            if s["glyph"] is not None:                           # a Line group: the oracle footprint of the kept points (exact)
                og = O.make_grid((self.g["min_x"], self.g["min_y"], self.g["max_x"], self.g["max_y"]), cell=(self.g["cs"], -self.g["cs"]),
                                 tile=(self.g["tw"], self.g["th"]))
                gl = O.make_glyph(O.GLYPH_LINE, half_length=s["glyph"]["hl"], max_radius=s["glyph"]["maxr"])
                for p, rt in ((0, O.SUM), (1, O.COUNT)):
                    if ok.any():
                        band = np.nan_to_num(O.run(og, rt, c["x"][ok], c["y"][ok], v[ok], glyph=gl, direction=c["dir"][ok])).reshape(-1)
                        pl[p][:] = (pl[p].astype(np.float64) + band.astype(np.float64)).astype(np.float32)
                continue
            pl[0][:] = (pl[0].astype(np.float64) + np.bincount(cell[ok], v[ok].astype(np.float64), self.W * self.H)).astype(np.float32)
            pl[1][:] = (pl[1].astype(np.float64) + np.bincount(cell[ok], minlength=self.W * self.H)).astype(np.float32)
            np.maximum.at(pl[2], cell[ok], v[ok])
            np.minimum.at(pl[3], cell[ok], v[ok])

    def touched_cells(self):
        g = self.g
        return np.repeat(np.repeat(self.touched, g["th"], 0), g["tw"], 1)[:self.H, :self.W].reshape(-1)

    def raw_bands(self):
        live = self.touched_cells()
        out = []
        for s, pl in zip(self.specs, self.planes):
            if s["type"] == "MostRecent":
                band = band_of_words(pl, (self.W * self.H,))
            else:
                sm, ct, mx, mn = pl
                with np.errstate(all="ignore"):
                    band = {"Sum": lambda: sm.copy(), "Count": lambda: np.where(ct > 0, ct, np.float32(np.nan)),
                            "Average": lambda: np.where(ct > 0, sm / ct, np.float32(np.nan)),
                            "WeightedAverage": lambda: np.where(ct > 0, sm / ct, np.float32(np.nan)),
                            "Max": lambda: np.where(mx == -FLT_MAX, np.float32(np.nan), mx),
                            "Min": lambda: np.where(mn == FLT_MAX, np.float32(np.nan), mn)}[s["type"]]()
            out.append(np.where(live, band, np.float32(np.nan)).astype(np.float32).reshape(self.H, self.W))
        return out


def assert_model(p, model, what):
    got, want = bands(p), model.raw_bands()
    assert len(got) == len(want)
    for b, (u, w) in enumerate(zip(got, want)):
        assert_bits(u, w, f"{what}: band {b} ({model.specs[b]['type']} of {model.specs[b]['ch']} under {model.specs[b]['filt']})")
    st = p.stats()
    assert (st.points_processed, st.collections_processed) == (model.survivors, model.collections), what


# ---- the cases, on either engine ---------------------------------------------------------------------------------------------------
CLASS2 = [("cls", "Equal", 2.0)]
FIRST = [("ret", "Equal", 1.0)]
MIXED = [S("Min", filt=CLASS2), S("Sum", filt=CLASS2), S("Count", filt=CLASS2),            # one group
         S("Max", filt=FIRST), S("Average", filt=FIRST),                                   # one group
         S("Average"),                                                                     # unfiltered
         S("MostRecent", filt=[("cls", "InSet", [2.0, 5.0])]),
         S("Sum", ch="t", filt=[("ret", "GreaterEqual", 2.0)]), S("Max", ch="t", filt=[("ret", "GreaterEqual", 2.0)])]
MIXED_GROUPS = [0, 0, 0, 1, 1, 2, 3, 4, 4]
ALL_FILTERED = [S("Sum", filt=CLASS2), S("Count", filt=CLASS2), S("Max", filt=FIRST), S("MostRecent", filt=CLASS2)]


def run_case(mode, specs, cfg_filt, n, seed, g=GRID, **kw):
    c = make_points(n, seed, g)
    model = Model(specs, cfg_filt, g)
    p = create(mode, specs, cfg_filt, g, **kw)
    p.ingest(make_cloud(c, mode))
    p.finalize()
    model.ingest(c)
    return p, model, c


def check_mixed(mode, n, tmp_path=None, **kw):
    p, model, c = run_case(mode, MIXED, (), n, 100 + n, **kw)
    if mode == "gpu":
        assert list(p.reduction_groups()) == MIXED_GROUPS
    assert_model(p, model, f"mixed pipeline, {n} points, {mode}")
    if mode == "gpu" and tmp_path is not None:
        # The grouping plan is one: a checkpoint the out-of-core driver writes from its parked planes (planes[4 g + p], two
        # bands under this budget: test_gpu_reduction_filters.py::test_out_of_core_row_bands) is the in-core pipeline's own
        ck = str(tmp_path / "ck")
        banded = create(mode, MIXED, (), gpu_memory_budget=60000, host_cache_budget=1 << 20, state_dir=str(tmp_path), **kw)
        assert banded.out_of_core()
        banded.ingest(make_cloud(c, "cpu"))
        banded.save_state(ck)
        q = create(mode, MIXED, (), state_dir=ck, resume=True, **kw)
        assert not q.out_of_core()
        q.finalize()
        for b, (u, w) in enumerate(zip(bands(q), bands(p))):
            assert_bits(u, w, f"band {b}: saved out of core, loaded in core, against the in-core pipeline, {n} points")
    return p


# PipelineConfig.filter alone: class 0 of the plan through the same sweep, at the sizes where that kernel changes shape (below,
# at and past one 4-point group, one 64-lane wave, one 256-thread workgroup plus a tail).
CFG_ONLY_SPECS = [S("Sum"), S("Count"), S("Min"), S("MostRecent")]
CFG_ONLY_SIZES = (1, 3, 4, 5, 63, 64, 65, 259, 1027)
CFG_ONLY_NONE = [("ret", "Greater", 7.0)]
CFG_ONLY_PREDS = {
    "one": [("ret", "LessEqual", 2.0)],
    "the same twice": [("ret", "LessEqual", 2.0), ("ret", "LessEqual", 2.0)],                       # (the table collapses it)
    "five channels": [("a", "GreaterEqual", -6.0), ("t", "Less", 5.0), ("cls", "NotEqual", 6.0), ("ret", "LessEqual", 2.0),
                      ("q", "GreaterEqual", 2.0)],                                                  # (a NaN in q fails)
    "sixteen": [("a", "NotEqual", k / 8.0) for k in range(12)] + [("t", "NotEqual", 0.0), ("ret", "LessEqual", 2.0),
                                                                  ("cls", "NotEqual", 1.0), ("q", "NotInSet", [1.0])],
    "none": CFG_ONLY_NONE,
}
SEVENTEEN = CFG_ONLY_PREDS["sixteen"] + [("t", "NotEqual", 1.0)]


def cfg_only_points(n):
    return make_points(n, 600 + n)


def check_cfg_filter_only(mode, n, preds, resident="device", **kw):
    c = cfg_only_points(n)
    model = Model(CFG_ONLY_SPECS, preds)
    p = create(mode, CFG_ONLY_SPECS, preds, **kw)
    p.ingest(make_cloud(c, mode if resident == "device" else "cpu"))
    p.finalize()
    model.ingest(c)
    what = f"cfg.filter alone ({len(preds)} predicates), {n} points, {mode}, {resident}-resident cloud"
    assert_model(p, model, what)
    assert p.stats().points_processed == model.survivors == int(conj_mask(c, preds).sum()), what
    if preds is CFG_ONLY_NONE:                                   # a successful no-op
        assert (p.stats().points_processed, p.stats().collections_processed) == (0, 0), what
        assert all(np.isnan(b).all() for b in bands(p)), what
    return p


def check_cfg_filter_too_long(mode):
    """17 predicates in PipelineConfig.filter: create refuses nothing; the device refuses the cloud at ingest, before any state
    changes (the host engine has no such limit and ingests it)."""
    import pytest
    c = cfg_only_points(259)
    p = create(mode, CFG_ONLY_SPECS, SEVENTEEN)
    if mode == "cpu":
        p.ingest(make_cloud(c, mode))
        p.finalize()
        model = Model(CFG_ONLY_SPECS, SEVENTEEN)
        model.ingest(c)
        assert_model(p, model, "17 predicates on the host engine")
        return
    with pytest.raises(RuntimeError, match="filter_points: more than 16 predicates"):
        p.ingest(make_cloud(c, mode))
    assert (p.stats().points_processed, p.stats().collections_processed) == (0, 0)
    p.finalize()
    assert all(np.isnan(b).all() for b in bands(p))


def check_all_filtered(mode, n, **kw):
    """No cfg.filter, every spec filtered: the flags come from every in-bounds point (the touch pass on the HIP engine)."""
    p, model, c = run_case(mode, ALL_FILTERED, (), n, 200 + n, **kw)
    assert_model(p, model, f"all specs filtered, {n} points, {mode}")
    if n >= 1027:
        got = bands(p)[0]                                        # Sum of `a` over class 2
        assert model.touched[0, 1] and not model.touched[1, 2]
        only5 = got[0:16, 16:32]                                 # tile (0, 1): class 5 only
        assert np.array_equal(only5.view(np.uint32), np.zeros_like(only5).view(np.uint32)), "a filtered Sum is 0.0 where only other classes fell"
        assert np.isnan(got[16:24, 32:40]).all(), "... and NaN in a tile nothing touched"
    if mode == "gpu":
        parent = create(mode, ALL_FILTERED[:1] + [S("Count", ch="t")], (), **kw)     # an unfiltered Count sets the flags by its scatter
        parent.ingest(make_cloud(c, mode))
        assert np.array_equal(read_touched(p), read_touched(parent))
        assert np.array_equal(read_touched(p), model.touched)
    return p


def check_with_cfg_filter(mode, n, **kw):
    cfg_filt = [("ret", "LessEqual", 2.0)]
    p, model, c = run_case(mode, MIXED, cfg_filt, n, 300 + n, **kw)
    assert_model(p, model, f"cfg.filter and spec filters, {n} points, {mode}")
    assert p.stats().points_processed == int((c["ret"] <= 2.0).sum())
    # a cfg.filter that keeps nothing: not a collection, nothing changes
    q = create(mode, ALL_FILTERED, [("ret", "Greater", 7.0)], **kw)
    q.ingest(make_cloud(c, mode))
    assert (q.stats().points_processed, q.stats().collections_processed) == (0, 0)
    q.finalize()
    assert all(np.isnan(b).all() for b in bands(q))


def check_predicate_edges(mode, n=1027, **kw):
    sixteen = [float(v) for v in range(16)]
    specs = [S("Count", filt=[("q", op, [2.0, 5.0] if "Set" in op else 2.0)]) for op in OPS]          # NaNs in q under every operator: eight filters
    p, model, c = run_case(mode, specs, (), n, 400 + n, **kw)
    assert np.isnan(c["q"]).any()
    assert_model(p, model, f"a NaN channel value under the eight operators, {mode}")
    specs = [S("Sum", ch="t", filt=[("cls", "InSet", sixteen)]),                                       # keeps everything
             S("Sum", ch="t"),
             S("Sum", filt=[("cls", "Greater", 99.0)]), S("Max", filt=[("cls", "Greater", 99.0)]),     # keeps nothing
             S("Count", filt=[("cls", "Greater", 99.0)]), S("MostRecent", filt=[("cls", "Greater", 99.0)])]
    p, model, _ = run_case(mode, specs, (), n, 400 + n, **kw)
    assert_model(p, model, f"a 16-entry set, a class that keeps everything, one that keeps nothing, {mode}")
    got = bands(p)
    assert_bits(got[0], got[1], "a class that keeps everything equals the unfiltered spec")
    live = model.touched_cells().reshape(model.H, model.W)
    assert (got[2][live] == 0.0).all() and np.isnan(got[2][~live]).all(), "a class that keeps nothing: Sum 0 in touched tiles"
    assert all(np.isnan(got[b]).all() for b in (3, 4, 5))
    nan_q = np.isnan(c["q"])
    for b, op in enumerate(OPS):                                 # a NaN passes NotEqual and NotInSet only
        assert pred_mask(c, ("q", op, [2.0, 5.0] if "Set" in op else 2.0))[nan_q].all() == (op in ("NotEqual", "NotInSet"))


def check_against_own_pipelines(mode, n=1027, **kw):
    """One tile that every class hits: a filtered spec's band is, bit for bit, the band of a pipeline of its own whose
    cfg.filter is the conjunction."""
    g, cfg_filt = ONE_TILE, [("ret", "LessEqual", 2.0)]
    specs = [S("Sum", filt=CLASS2), S("Min", filt=CLASS2), S("Average", filt=[("cls", "NotEqual", 2.0), ("t", "Less", 4.0)]),
             S("MostRecent", filt=[("cls", "InSet", [1.0, 6.0])]), S("Count")]
    c = make_points(n, 500 + n, g, clustered=False)
    p = create(mode, specs, cfg_filt, g, **kw)
    p.ingest(make_cloud(c, mode))
    p.finalize()
    got = bands(p)
    for b, s in enumerate(specs):
        assert conj_mask(c, cfg_filt + s["filt"]).any()
        own = create(mode, [S(s["type"], s["ch"])], cfg_filt + s["filt"], g, **kw)
        own.ingest(make_cloud(c, mode))
        own.finalize()
        assert_bits(got[b], bands(own)[0], f"spec {b} against a pipeline of its own, {mode}")


def check_refusals(mode):
    def refused(specs, cfg_filt, message):
        assert pcr.Pipeline.create(make_config(mode, specs, cfg_filt)) is None
        assert message in pcr.pipeline_create_error(), pcr.pipeline_create_error()
    refused([S("Sum", filt=[("cls", "Equal", float(k))]) for k in range(9)], (), "more than 8 distinct reduction filters")
    assert pcr.Pipeline.create(make_config(mode, [S("Sum", filt=[("cls", "Equal", float(k))]) for k in range(8)])) is not None
    refused([S("Sum", filt=[("cls", "NotEqual", float(k)) for k in range(16)])], [("ret", "Less", 9.0)], "together hold more than 16 predicates")
    assert pcr.Pipeline.create(make_config(mode, [S("Sum", filt=[("cls", "NotEqual", float(k)) for k in range(16)])])) is not None
    refused([S("Sum", filt=[("cls", "NotEqual", float(100 * j + k)) for k in range(11)]) for j in range(3)], (),
            "more than 32 distinct filter predicates")
    # at ingest: a spec filter on a missing or non-Float32 channel, and the state is untouched afterwards
    import pytest
    c = make_points(65, 7)
    specs = [S("Sum"), S("Count", filt=[("nope", "Equal", 1.0)])]
    p = create(mode, specs)
    with pytest.raises(RuntimeError, match="filter_points: channel not found: nope"):
        p.ingest(make_cloud(c, mode))
    cloud = make_cloud(c, "cpu")
    cloud.add_channel("nope", pcr.DataType.Int32)
    with pytest.raises(RuntimeError, match="filter_points: only Float32 channels supported for filtering"):
        p.ingest(cloud.to_device() if mode == "gpu" else cloud)
    assert (p.stats().points_processed, p.stats().collections_processed) == (0, 0)
    p.finalize()
    assert all(np.isnan(b).all() for b in bands(p))


def check_two_ingests_and_checkpoint(mode, tmp_path, **kw):
    specs, cfg_filt = MIXED[:7], [("ret", "LessEqual", 2.0)]
    model = Model(specs, cfg_filt)
    p = create(mode, specs, cfg_filt, **kw)
    c1, c2 = make_points(1027, 61), make_points(700, 62)
    p.ingest(make_cloud(c1, mode))
    model.ingest(c1)
    p.finalize()
    assert_model(p, model, f"first ingest, {mode}")
    p.ingest(make_cloud(c2, mode))
    model.ingest(c2)
    p.finalize()
    assert_model(p, model, f"second ingest behind a finalize, {mode}")
    ck = str(tmp_path / "ck")
    p.save_state(ck)
    q = create(mode, specs, cfg_filt, state_dir=ck, resume=True, **kw)       # checkpoints record no filter: the configuration does
    c3 = make_points(333, 63)
    q.ingest(make_cloud(c3, mode))
    q.finalize()
    model.survivors = model.collections = 0
    model.ingest(c3)
    assert_model(q, model, f"resumed in a new pipeline, {mode}")


def las_case(tmp_path):
    """A LAS 1.4 file (format 6) whose classification no reduction names: (path, the model's cloud)."""
    import las_common as LC
    n, fmt = 3000, 6
    rng = np.random.default_rng(9)
    f = LC.make_fields(fmt, n, rng)
    f["X"] = rng.integers(1000, (GRID["W"] - 1) * 1000, n).astype(np.int32)
    f["Y"] = rng.integers(1000, (GRID["H"] - 1) * 1000, n).astype(np.int32)
    f["Z"] = rng.integers(-400, 8000, n).astype(np.int32)
    f["classification"] = (np.arange(n) % 5).astype(np.uint8)
    scale, offset = (0.001, 0.001, 0.125), (0.0, 0.0, 0.0)
    path = os.path.join(str(tmp_path), "classified.las")
    LC.write_las(path, fmt, LC.pack_records(fmt, f), scale, offset, version=(1, 4))
    want = LC.expected(fmt, f, scale, offset)
    return path, dict(x=want["x"], y=want["y"], z=want["z"], classification=want["classification"])


def check_las(mode, tmp_path):
    path, c = las_case(tmp_path)
    specs = [S("Min", ch="z", filt=[("classification", "Equal", 2.0)]), S("Max", ch="z")]
    p = create(mode, specs)
    assert p.ingest_file(path, 1024) == len(c["x"])
    p.finalize()
    model = Model(specs)
    model.ingest(c)
    got, want = bands(p), model.raw_bands()
    for b in range(2):
        assert_bits(got[b], want[b], f"LAS band {b}, {mode}")
    assert not np.array_equal(np.isnan(got[0]), np.isnan(got[1]))            # (the filter removed something)


LINE = dict(kind="line", hl=3.0, maxr=6.0)


def line_points(n, seed):
    c = make_points(n, seed)
    c["dir"] = (np.random.default_rng(seed + 1).integers(0, 8, n) * (np.pi / 8.0)).astype(np.float32)
    c["a"] = np.abs(c["a"])
    return c


def check_line(mode, n=1027, **kw):
    specs = [S("Sum", filt=CLASS2, glyph=LINE), S("Count", filt=CLASS2, glyph=LINE), S("Count", glyph=LINE)]
    c = line_points(n, 71)
    p = create(mode, specs, **kw)
    if mode == "gpu":
        assert list(p.reduction_groups()) == [0, 0, 1]
    p.ingest(make_cloud(c, mode))
    p.finalize()
    model = Model(specs)
    model.ingest(c)
    assert_model(p, model, f"filtered Line groups, {mode}")
