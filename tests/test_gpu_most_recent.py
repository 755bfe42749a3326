"""ReductionType.MostRecent on the MI355X: the C-ABI entry points (pcr_hip_scatter_select on both paths, select_pack /
unpack / merge, state_init / state_merge of type 8, finalize_select) and the Pipeline on the HIP engine -- host and device
clouds, ingest_file, beside Average / Max of the same channel, out of core, row-block shards, ExecutionMode.CPU, checkpoints
across the engines, and one full-size case.  Everything BIT FOR BIT against the NumPy model of the contract
(tests/most_recent_common.py): a selection copies bits, and the fold is associative, commutative and idempotent."""
import ctypes as C
import os

import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
from conftest import load_cabi

import most_recent_common as M

pytestmark = pytest.mark.gpu

T = pcr.ReductionType
GPU = pcr.ExecutionMode.GPU


@pytest.fixture(scope="module")
def A():
    mod = load_cabi()
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


class SelectRun:
    """One MostRecent group driven purely through the C-ABI: a packed plane + an engine."""

    def __init__(self, A, grid, path, define=True):
        self.A, self.L, self.grid = A, A.lib(), grid
        self.cells = grid.state_rows * grid.width
        self.packed = A.DeviceBuffer(self.cells * 8)
        if define:
            A.check(self.L.pcr_hip_memset(self.packed.ptr, 0, self.cells * 8, None))
        else:                                           # garbage: planes_fresh = 2 must define every word
            A.check(self.L.pcr_hip_memset(self.packed.ptr, 0xA5, self.cells * 8, None))
        self.engine = C.c_void_p()
        A.check(self.L.pcr_hip_engine_create(C.byref(self.engine), C.byref(grid), 0, None))
        A.check(self.L.pcr_hip_engine_set_path(self.engine, path))

    def scatter(self, x, y, v, t, fresh=0, mask=None):
        A, L = self.A, self.L
        bufs = [A.DeviceBuffer.from_numpy(np.asarray(a, dtype=d)) for a, d in
                ((x, np.float64), (y, np.float64), (v, np.float32), (t, np.float32))]
        mb = None
        if mask is not None:
            mb = A.DeviceBuffer.from_numpy(np.asarray(mask, dtype=np.uint8))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, mb.ptr if mb else None))
        A.check(L.pcr_hip_engine_planes_fresh(self.engine, fresh))
        A.check(L.pcr_hip_scatter_select(self.engine, self.packed.ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, len(x)))
        A.check(L.pcr_hip_stream_synchronize(None))
        A.check(L.pcr_hip_engine_set_point_mask(self.engine, None))

    def stats(self):
        st = self.A.ScatterStats()
        self.A.check(self.L.pcr_hip_engine_stats(self.engine, C.byref(st)))
        return st

    def words(self):
        return self.packed.to_numpy(np.uint64, (self.cells,))

    def finalize(self):
        A, L = self.A, self.L
        rows = self.grid.own_row1 - self.grid.own_row0
        out = A.DeviceBuffer(rows * self.grid.width * 4)
        p, tx, ty = C.c_void_p(), C.c_int32(0), C.c_int32(0)
        A.check(L.pcr_hip_engine_tile_touched(self.engine, C.byref(p), C.byref(tx), C.byref(ty)))
        A.check(L.pcr_hip_finalize_select(C.byref(self.grid), self.packed.ptr, p, out.ptr, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        return out.to_numpy(np.float32, (rows, self.grid.width))

    def close(self):
        self.L.pcr_hip_engine_destroy(self.engine)
        self.packed.free()


def cabi_grid(A, W, H, tile=(4096, 4096), own_rows=None):
    return A.make_grid((0.0, 0.0, float(W), float(H)), dims=(W, H), tile=tile, own_rows=own_rows)


@pytest.mark.parametrize("path", [1, 2, 0])
@pytest.mark.parametrize("fresh", [0, 1, 2])
def test_scatter_select_paths_and_fresh_hints(A, path, fresh):
    """Two scatters into one plane: the first with the hint under test (2: onto garbage), the second accumulating."""
    W, H = 300, 200                                      # not a multiple of the 128 x 128 LDS tile
    x, y, v, t = M.tricky_cloud(W, H, 40_000, seed=3)
    x2, y2, v2, t2 = M.tricky_cloud(W, H, 30_000, seed=4, stamps="ties")
    og = M.oracle_grid(W, H, tile=(64, 64))
    c1, c2 = M.cells_oracle(og, x, y), M.cells_oracle(og, x2, y2)
    run = SelectRun(A, cabi_grid(A, W, H, tile=(64, 64)), path, define=fresh != 2)
    try:
        run.scatter(x, y, v, t, fresh=fresh)
        st = run.stats()
        assert st.points_valid == int((c1 >= 0).sum()) and st.points_in == len(x)
        assert st.path == (0 if path == 1 else 1)
        words = M.fold_words(c1, v, t, W * H)
        assert np.array_equal(run.words(), words), "state words after the first scatter"
        run.scatter(x2, y2, v2, t2)
        M.fold_words(c2, v2, t2, W * H, words=words)
        assert np.array_equal(run.words(), words), "state words after the second scatter"
        M.assert_bits(run.finalize(), M.band_of_words(words, (H, W)), f"path {path}, fresh {fresh}")
    finally:
        run.close()


@pytest.mark.parametrize("path", [1, 2])
def test_point_mask_and_own_rows(A, path):
    W, H = 256, 192
    x, y, v, t = M.tricky_cloud(W, H, 30_000, seed=8, stamps="ties")
    keep = np.random.default_rng(1).integers(0, 2, len(x)).astype(np.uint8)
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    r0, r1 = 50, 130
    run = SelectRun(A, cabi_grid(A, W, H, own_rows=(r0, r1)), path)
    try:
        run.scatter(x, y, v, t, mask=keep)
        row = cell // W
        own = (cell >= 0) & (row >= r0) & (row < r1) & (keep != 0)
        want = M.model_band(np.where(own, cell, -1), v, t, (H, W))[r0:r1]
        M.assert_bits(run.finalize(), want, "masked, row block")
        assert run.stats().points_valid == int(own.sum())
    finally:
        run.close()


@pytest.mark.parametrize("skew", [0, 1])
def test_ragged_and_unaligned_channel_arrays(A, skew):
    """A point count that is no multiple of 4, and value / key arrays that start 4 bytes off a 16-byte boundary."""
    W, H, n = 300, 200, 40_003
    x, y, v, t = M.tricky_cloud(W, H, n, seed=13, stamps="ties")
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    run = SelectRun(A, cabi_grid(A, W, H), 2)
    try:
        L = A.lib()
        dx, dy = A.DeviceBuffer.from_numpy(x), A.DeviceBuffer.from_numpy(y)
        dv = A.DeviceBuffer.from_numpy(np.concatenate([np.zeros(skew, np.float32), v]))
        dt = A.DeviceBuffer.from_numpy(np.concatenate([np.zeros(skew, np.float32), t]))
        A.check(L.pcr_hip_scatter_select(run.engine, run.packed.ptr, dx.ptr, dy.ptr, C.c_void_p(dv.ptr.value + 4 * skew),
                                         C.c_void_p(dt.ptr.value + 4 * skew), n))
        A.check(L.pcr_hip_stream_synchronize(None))
        M.assert_bits(run.finalize(), M.model_band(cell, v, t, (H, W)), f"skew {skew}")
    finally:
        run.close()


def test_hot_spot_splits_a_bin(A):
    """400 000 points inside one 128 x 128 LDS tile: more than 1 << 17 records, so the scan splits the bin and its items
    merge with the global 64-bit atomic max -- with every fresh hint."""
    W = H = 512
    rng = np.random.default_rng(12)
    n = 400_000
    x, y = rng.uniform(130, 250, n), rng.uniform(H - 250, H - 130, n)
    v = rng.normal(0, 5, n).astype(np.float32)
    t = rng.integers(0, 50, n).astype(np.float32)
    xb, yb = rng.uniform(0, W, 20_000), rng.uniform(0, H, 20_000)
    x, y = np.concatenate([x, xb]), np.concatenate([y, yb])
    v = np.concatenate([v, rng.normal(0, 5, 20_000).astype(np.float32)])
    t = np.concatenate([t, rng.integers(0, 50, 20_000).astype(np.float32)])
    want = M.model_band(M.cells_floor(x, y, W, H), v, t, (H, W))
    for fresh in (0, 1, 2):
        run = SelectRun(A, cabi_grid(A, W, H), 2, define=fresh != 2)
        try:
            run.scatter(x, y, v, t, fresh=fresh)
            M.assert_bits(run.finalize(), want, f"hot spot, fresh {fresh}")
        finally:
            run.close()


@pytest.mark.parametrize("mode", ["two_level", "bands"])
@pytest.mark.parametrize("fresh", [0, 2])
def test_large_grid_forms_on_a_small_grid(A, monkeypatch, mode, fresh):
    monkeypatch.setenv("PCR_HIP_DEBUG_MAX_BINS", "6")          # read by pcr_hip_engine_create
    monkeypatch.setenv("PCR_HIP_DEBUG_TWO_LEVEL", "1" if mode == "two_level" else "0")
    W, H = 640, 520                                            # 5 x 5 LDS tiles: more than 6 bins
    x, y, v, t = M.tricky_cloud(W, H, 60_000, seed=17, stamps="ties")
    cell = M.cells_oracle(M.oracle_grid(W, H, tile=(256, 256)), x, y)
    run = SelectRun(A, cabi_grid(A, W, H, tile=(256, 256)), 2, define=fresh != 2)
    try:
        run.scatter(x, y, v, t, fresh=fresh)
        assert run.stats().path == 1 and run.stats().num_bins == 25
        M.assert_bits(run.finalize(), M.model_band(cell, v, t, (H, W)), f"{mode}, fresh {fresh}")
    finally:
        run.close()


def test_pack_unpack_merge_and_state_ops(A):
    L = A.lib()
    n = 10_001                                                 # odd: the 16-byte bodies have a tail
    rng = np.random.default_rng(6)
    special = np.float32([np.nan, -np.inf, -M.FLT_MAX, np.inf, 0.0, -0.0, 7.0])

    def planes(seed):
        r = np.random.default_rng(seed)
        v = r.normal(0, 3, n).astype(np.float32)
        v[r.integers(0, n, 200)] = np.nan
        t = r.integers(-3, 3, n).astype(np.float32)
        idx = r.integers(0, n, n // 3)
        t[idx] = special[r.integers(0, len(special), len(idx))]
        return v, t

    def words_of(v, t):
        return np.where(M.accepted(t), M.word(t, v), np.uint64(0))

    va, ta = planes(1)
    vb, tb = planes(2)
    wa, wb = words_of(va, ta), words_of(vb, tb)
    dv, dt = A.DeviceBuffer.from_numpy(va), A.DeviceBuffer.from_numpy(ta)
    pa, pb = A.DeviceBuffer(n * 8), A.DeviceBuffer(n * 8)
    A.check(L.pcr_hip_select_pack(dv.ptr, dt.ptr, pa.ptr, n, None))
    assert np.array_equal(pa.to_numpy(np.uint64, (n,)), wa)
    ov, ot = A.DeviceBuffer(n * 4), A.DeviceBuffer(n * 4)
    A.check(L.pcr_hip_select_unpack(pa.ptr, ov.ptr, ot.ptr, n, None))
    val, ts = M.state_of_words(wa, (n,))
    assert np.array_equal(ov.to_numpy(np.uint32, (n,)), val.view(np.uint32))
    assert np.array_equal(ot.to_numpy(np.uint32, (n,)), ts.view(np.uint32))
    A.check(L.pcr_hip_select_pack(ov.ptr, ot.ptr, pb.ptr, n, None))            # round trip
    assert np.array_equal(pb.to_numpy(np.uint64, (n,)), wa)
    # elementwise 64-bit max
    pb2 = A.DeviceBuffer.from_numpy(wb)
    A.check(L.pcr_hip_select_merge(pa.ptr, pb2.ptr, n, None))
    assert np.array_equal(pa.to_numpy(np.uint64, (n,)), np.maximum(wa, wb))
    # state_init / state_merge of type 8 on the two float planes
    sa, sb = A.DeviceBuffer(2 * n * 4), A.DeviceBuffer.from_numpy(np.concatenate([vb, tb]))
    A.check(L.pcr_hip_state_init(A.MOST_RECENT, sa.ptr, n, None))
    st = sa.to_numpy(np.uint32, (2, n))
    assert (st[0] == 0x7FC00000).all() and (st[1].view(np.float32) == -M.FLT_MAX).all()
    A.check(L.pcr_hip_state_merge(A.MOST_RECENT, sa.ptr, sb.ptr, n, None))
    val, ts = M.state_of_words(wb, (n,))
    st = sa.to_numpy(np.uint32, (2, n))
    assert np.array_equal(st[0], val.view(np.uint32)) and np.array_equal(st[1], ts.view(np.uint32))
    sa2 = A.DeviceBuffer.from_numpy(np.concatenate([va, ta]))
    A.check(L.pcr_hip_state_merge(A.MOST_RECENT, sa.ptr, sa2.ptr, n, None))
    val, ts = M.state_of_words(np.maximum(wa, wb), (n,))
    st = sa.to_numpy(np.uint32, (2, n))
    assert np.array_equal(st[0], val.view(np.uint32)) and np.array_equal(st[1], ts.view(np.uint32))
    # the functions that take pcr_hip_planes refuse the type
    g = cabi_grid(A, 16, 16)
    pl = A.Planes()
    out = A.DeviceBuffer(16 * 16 * 4)
    assert L.pcr_hip_finalize(A.MOST_RECENT, C.byref(g), C.byref(pl), None, out.ptr, None) == 1
    rt = (C.c_int * 1)(A.MOST_RECENT)
    outs = (C.c_void_p * 1)(out.ptr.value)
    assert L.pcr_hip_finalize_group(C.byref(g), C.byref(pl), None, 1, rt, outs, None) == 1


# ---- the Pipeline ---------------------------------------------------------------------------------------------------

def gpu_cfg(W, H, tile=None, reductions=None, **kw):
    cfg = M.make_cfg(W, H, tile=tile, mode=GPU)
    cfg.reductions = reductions or [M.most_recent_spec()]
    for k, val in kw.items():
        setattr(cfg, k, val)
    return cfg


def create(cfg, engine="hip"):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == engine
    return p


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("scatter_path", [0, 1, 2])
def test_pipeline_host_and_device_clouds(where, scatter_path):
    W, H = 400, 260
    parts = [M.tricky_cloud(W, H, 50_000, seed=s, stamps="ties" if s == 42 else "mixed") for s in (41, 42)]
    og = M.oracle_grid(W, H, tile=(128, 128))
    p = create(gpu_cfg(W, H, tile=(128, 128), scatter_path=scatter_path))
    words = np.zeros(W * H, dtype=np.uint64)
    for x, y, v, t in parts:
        cloud = M.make_cloud(x, y, value=v, time=t)
        p.ingest(cloud.to_device() if where == "device" else cloud)
        M.fold_words(M.cells_oracle(og, x, y), v, t, W * H, words=words)
    p.finalize()
    M.assert_bits(M.bands(p)[0], M.band_of_words(words, (H, W)), f"{where}, path {scatter_path}")
    assert p.last_scatter()["bands_with_scatter"] == 0
    # finalize changes no state; an empty pipeline is all NaN
    p.finalize()
    M.assert_bits(M.bands(p)[0], M.band_of_words(words, (H, W)), "second finalize")
    e = create(gpu_cfg(W, H))
    e.finalize()
    assert np.isnan(M.bands(e)[0]).all()


def test_filter_and_errors_on_the_hip_engine():
    W, H, n = 200, 150, 30_000
    x, y, v, t = M.tricky_cloud(W, H, n, seed=23)
    cls = np.random.default_rng(2).integers(0, 4, n).astype(np.float32)
    f = pcr.FilterSpec()
    f.add("cls", pcr.CompareOp.GreaterEqual, 2.0)
    p = create(gpu_cfg(W, H, filter=f))
    with pytest.raises(RuntimeError, match="pipeline: timestamp channel not found: time"):
        p.ingest(M.make_cloud(x, y, value=v, cls=cls))
    p.ingest(M.make_cloud(x, y, value=v, time=t, cls=cls))
    p.finalize()
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    M.assert_bits(M.bands(p)[0], M.model_band(cell, v, t, (H, W), keep=cls >= 2.0), "filtered")
    assert pcr.Pipeline.create(gpu_cfg(8, 8, reductions=[M.most_recent_spec(stamp="")])) is None
    assert pcr.pipeline_create_error() == "pipeline: MostRecent requires a timestamp_channel"
    line = pcr.line_splat_spec("value", default_direction=0.3, default_half_length=2.0, max_radius_cells=4.0)
    line.type, line.timestamp_channel = T.MostRecent, "time"
    q = create(gpu_cfg(W, H, reductions=[line]))
    with pytest.raises(RuntimeError, match="glyph splatting only supports"):
        q.ingest(M.make_cloud(x, y, value=v, time=t))


def test_ingest_file_in_chunks(tmp_path):
    W, H, n = 300, 300, 200_000
    x, y, v, t = M.tricky_cloud(W, H, n, seed=29, stamps="ties")
    path = str(tmp_path / "stamped.pcrp")
    pcr.write_point_cloud(path, M.make_cloud(x, y, value=v, time=t))
    p = create(gpu_cfg(W, H, tile=(128, 128)))
    assert p.ingest_file(path, chunk_points=33_000) == n          # 7 chunks, the last one ragged
    p.finalize()
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    M.assert_bits(M.bands(p)[0], M.model_band(cell, v, t, (H, W)), "ingest_file")


def test_beside_average_and_max_of_the_same_channel():
    W, H, n = 512, 384, 300_000
    rng = np.random.default_rng(33)
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    v = rng.normal(0, 10, n).astype(np.float32)
    t = rng.integers(0, 20, n).astype(np.float32)
    cloud = M.make_cloud(x, y, value=v, time=t).to_device()
    both = create(gpu_cfg(W, H, reductions=[M.spec(T.Average), M.most_recent_spec(), M.spec(T.Max)]))
    alone = create(gpu_cfg(W, H, reductions=[M.spec(T.Average), M.spec(T.Max)]))
    for p in (both, alone):
        p.ingest(cloud)
        p.finalize()
    b, a = M.bands(both), M.bands(alone)
    M.assert_bits(b[0], a[0], "Average beside MostRecent")
    M.assert_bits(b[2], a[1], "Max beside MostRecent")
    M.assert_bits(b[1], M.model_band(M.cells_floor(x, y, W, H), v, t, (H, W)), "MostRecent beside them")


@pytest.mark.parametrize("sign,rtype", [(1.0, O.MAX), (-1.0, O.MIN)])
def test_against_the_oracles_max_and_min(sign, rtype):
    W, H, n = 256, 256, 200_000
    rng = np.random.default_rng(9)
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    v = rng.uniform(0.5, 100.0, n).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)
    og = M.oracle_grid(W, H)
    want, count = O.run(og, rtype, x, y, v), O.run(og, O.COUNT, x, y, v)
    p = create(gpu_cfg(W, H))
    p.ingest(M.make_cloud(x, y, value=v, time=np.float32(sign) * v))
    p.finalize()
    got = M.bands(p)[0]
    m = count > 0
    assert m.any() and np.array_equal(np.isnan(got), ~m)
    assert np.array_equal(got[m].view(np.uint32), np.asarray(want, dtype=np.float32)[m].view(np.uint32))


def test_out_of_core_in_three_bands_or_more(tmp_path):
    W, H = 256, 1024
    parts = [M.tricky_cloud(W, H, 80_000, seed=s, stamps="ties") for s in (51, 52)]
    og = M.oracle_grid(W, H, tile=(256, 256))
    # MostRecent (8 B) + Count (4 B) + two bands (8 B) = 20 B per cell = 5 KB per row, 1.25 MB per 256-row tile row
    reds = [M.most_recent_spec(), M.spec(T.Count)]
    ooc = pcr.Pipeline.create(gpu_cfg(W, H, tile=(256, 256), reductions=reds, gpu_memory_budget=3 << 19, host_cache_budget=1,
                                      state_dir=str(tmp_path)))
    assert ooc is not None and ooc.out_of_core() and ooc.engine() == "hip"
    words = np.zeros(W * H, dtype=np.uint64)
    for x, y, v, t in parts:
        ooc.ingest(M.make_cloud(x, y, value=v, time=t))
        M.fold_words(M.cells_oracle(og, x, y), v, t, W * H, words=words)
    spilled = [n for n in os.listdir(ooc.spill_dir())]
    assert spilled, "host_cache_budget = 1 byte: every band goes through its .pcrt files"
    ooc.finalize()
    got = M.bands(ooc)
    M.assert_bits(got[0], M.band_of_words(words, (H, W)), "out of core")
    x = np.concatenate([p[0] for p in parts]); y = np.concatenate([p[1] for p in parts])
    M.assert_bits(got[1], O.run(og, O.COUNT, x, y, np.zeros(len(x), np.float32)), "Count beside it, out of core")
    row, col, st, rt = pcr.read_tile_state(os.path.join(ooc.spill_dir(), "reduction_0", "tile_0002_0000.pcrt"))
    assert rt == T.MostRecent and st.shape == (2, 256, 256)
    val, ts = M.state_of_words(words, (H, W))
    assert np.array_equal(st[0].view(np.uint32), val[512:768].view(np.uint32))
    assert np.array_equal(st[1].view(np.uint32), ts[512:768].view(np.uint32))


def test_two_row_block_shards_on_one_gpu():
    """Two row-block pipelines (as two ranks would hold): a Point glyph reaches no apron row, so the bands stacked are the
    unsharded ones; state_planes() shows the group as its value / timestamp planes with reach 0."""
    W = H = 96
    x, y, v, t = M.tricky_cloud(W, H, 20_000, seed=61, stamps="ties")
    gs = pcr.gaussian_splat_spec("value", default_sigma=2.0, max_radius_cells=5.0)
    cloud = M.make_cloud(x, y, value=v, time=t).to_device()
    shards = []
    for r0, r1 in ((0, 40), (40, 96)):
        p = create(gpu_cfg(W, H, reductions=[gs, M.most_recent_spec()], shard_row_begin=r0, shard_row_end=r1))
        p.ingest(cloud)
        p.synchronize()
        shards.append(p)
    top, bot = shards
    assert top.halo_rows() == 5 and bot.state_row_begin() == 35
    views, reach = top.state_planes(), top.plane_reach_rows()
    assert [(k, g) for _, k, g in views] == [(1, 0), (2, 0), (1, 1), (2, 1)] and list(reach) == [5, 5, 0, 0]
    for p in shards:
        p.finalize()
    got = np.vstack([M.bands(top)[1], M.bands(bot)[1]])
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    M.assert_bits(got, M.model_band(cell, v, t, (H, W)), "two shards stacked")
    # the snapshot is the state: value / timestamp planes of the top shard's window
    A = load_cabi()
    rows = top.state_row_count()
    snap = [np.empty((rows, W), np.float32) for _ in range(2)]
    for a, (ptr, _, _) in zip(snap, top.state_planes()[2:]):
        A.check(A.lib().pcr_hip_memcpy_d2h(a.ctypes.data, C.c_void_p(ptr), a.nbytes, None))
    A.check(A.lib().pcr_hip_device_synchronize())
    row = cell // W
    own = (cell >= 0) & (row < 40)
    val, ts = M.state_of_words(M.fold_words(np.where(own, cell, -1), v, t, W * H), (H, W))
    assert np.array_equal(snap[0].view(np.uint32), val[:rows].view(np.uint32))
    assert np.array_equal(snap[1].view(np.uint32), ts[:rows].view(np.uint32))


def test_cpu_mode_equals_the_hip_engine_and_checkpoints_cross(tmp_path):
    W, H = 200, 140
    x1, y1, v1, t1 = M.tricky_cloud(W, H, 40_000, seed=71)
    x2, y2, v2, t2 = M.tricky_cloud(W, H, 40_000, seed=72, stamps="ties")
    c1, c2 = M.make_cloud(x1, y1, value=v1, time=t1), M.make_cloud(x2, y2, value=v2, time=t2)
    og = M.oracle_grid(W, H, tile=(64, 64))
    words = M.fold_words(M.cells_oracle(og, x1, y1), v1, t1, W * H)
    M.fold_words(M.cells_oracle(og, x2, y2), v2, t2, W * H, words=words)
    want = M.band_of_words(words, (H, W))

    def cfg(mode):
        c = M.make_cfg(W, H, tile=(64, 64), mode=mode, threads=3)
        c.reductions = [M.most_recent_spec()]
        return c

    hip, host = create(cfg(GPU)), create(cfg(pcr.ExecutionMode.CPU), "host")
    for p in (hip, host):
        p.ingest(c1)
        p.ingest(c2)
        p.finalize()
    M.assert_bits(M.bands(hip)[0], want, "hip")
    M.assert_bits(M.bands(host)[0], M.bands(hip)[0], "host == hip")
    # a checkpoint written by one engine, resumed by the other -- both ways, the files byte for byte the same
    for writer, reader, tag in ((GPU, pcr.ExecutionMode.CPU, "hip_to_host"), (pcr.ExecutionMode.CPU, GPU, "host_to_hip")):
        d = str(tmp_path / tag)
        a = pcr.Pipeline.create(cfg(writer))
        a.ingest(c1)
        a.save_state(d)
        b = pcr.Pipeline.create(cfg(reader))
        b.load_state(d)
        b.ingest(c2)
        b.finalize()
        M.assert_bits(M.bands(b)[0], want, tag)
    for name in sorted(os.listdir(str(tmp_path / "hip_to_host"))):
        assert open(os.path.join(str(tmp_path / "hip_to_host"), name), "rb").read() == \
               open(os.path.join(str(tmp_path / "host_to_hip"), name), "rb").read(), name


def test_full_size_c2_shape_with_ties_everywhere():
    """C2's shape: 50 M uniform points on 4096 x 4096, timestamps drawn from 1 000 distinct values (every cell has ties),
    device-resident, against the model over all 16.8 M cells."""
    G, n = 4096, 50_000_000
    rng = np.random.default_rng(42)
    x, y = rng.uniform(2, G - 2, n), rng.uniform(2, G - 2, n)
    v = rng.uniform(0, 1, n).astype(np.float32)
    t = rng.integers(0, 1000, n).astype(np.float32)
    cloud = M.make_cloud(x, y, value=v, time=t).to_device()
    p = create(gpu_cfg(G, G))
    p.ingest(cloud)
    p.finalize()
    assert p.last_scatter()["path"] == "binned" and p.last_scatter()["points_valid"] == n
    got = M.bands(p)[0]
    del cloud
    cell = M.cells_floor(x, y, G, G)
    words = np.zeros(G * G, dtype=np.uint64)
    step = 10_000_000
    for i in range(0, n, step):
        M.fold_words(cell[i:i + step], v[i:i + step], t[i:i + step], G * G, words=words)
    M.assert_bits(got, M.band_of_words(words, (G, G)), "full size")
