"""ReductionType.MostRecent on the host engine (ExecutionMode.CPU): per cell the value of the point with the greatest
timestamp, ties broken by the greater value (include/pcr_hip.h "MostRecent").  Checked BIT FOR BIT against a NumPy model of
the contract (tests/most_recent_common.py), against a literal loop of the reference's combine_timestamped, and against the
frozen oracle's Max / Min bands.  No tolerance anywhere: a selection copies bits."""
import ctypes as C
import itertools
import os
import struct

import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
from pcr import _cabi as A

import most_recent_common as M

T = pcr.ReductionType


def run_host(cfg, clouds, reductions=None):
    cfg.reductions = reductions or [M.most_recent_spec()]
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "host"
    for c in clouds:
        pipe.ingest(c)
    pipe.finalize()
    return pipe


@pytest.mark.parametrize("threads", [1, 3, 8])
@pytest.mark.parametrize("stamps", ["mixed", "ties"])
def test_host_engine_equals_the_model(threads, stamps):
    """A multi-tile grid, Q1 points on the bounds, points outside, NaN / -inf / -FLT_MAX / +inf / +-0.0 timestamps (mixed) or
    integer timestamps 0..7 (ties: every cell decides by the value)."""
    W, H, n = 50, 37, 6000
    x, y, v, t = M.tricky_cloud(W, H, n, seed=11, stamps=stamps)
    og = M.oracle_grid(W, H, tile=(16, 16))
    cell = M.cells_oracle(og, x, y)
    assert (cell < 0).any() and (cell >= 0).sum() > n // 2
    want = M.model_band(cell, v, t, (H, W))
    pipe = run_host(M.make_cfg(W, H, tile=(16, 16), threads=threads), [M.make_cloud(x, y, value=v, time=t)])
    M.assert_bits(M.bands(pipe)[0], want, f"{stamps}, {threads} threads")
    if stamps == "mixed":
        assert np.isnan(want).any() and (~np.isnan(want)).any()


def test_reference_fold_in_both_orders_equals_the_model():
    """Distinct timestamps inside every cell: the reference's sequential combine_timestamped gives the model's band in any
    order -- this ties the contract to the reference's text."""
    W, H, n = 40, 40, 20_000
    rng = np.random.default_rng(5)
    x, y = rng.uniform(-1, W + 1, n), rng.uniform(-1, H + 1, n)
    v = rng.normal(0, 10, n).astype(np.float32)
    t = rng.permutation(n).astype(np.float32)                   # distinct, exactly representable
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    want = M.model_band(cell, v, t, (H, W))
    M.assert_bits(M.reference_loop(cell, v, t, (H, W), range(n)), want, "input order")
    M.assert_bits(M.reference_loop(cell, v, t, (H, W), range(n - 1, -1, -1)), want, "reversed")
    pipe = run_host(M.make_cfg(W, H), [M.make_cloud(x, y, value=v, time=t)])
    M.assert_bits(M.bands(pipe)[0], want, "host engine")


@pytest.mark.parametrize("sign,rtype", [(1.0, O.MAX), (-1.0, O.MIN)])
def test_timestamp_equal_to_the_value_gives_the_oracles_max_and_min(sign, rtype):
    W, H, n = 64, 48, 30_000
    rng = np.random.default_rng(9)
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    v = rng.uniform(0.5, 100.0, n).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)     # finite, non-zero
    og = M.oracle_grid(W, H, tile=(32, 32))
    want = O.run(og, rtype, x, y, v)
    count = O.run(og, O.COUNT, x, y, v)
    pipe = run_host(M.make_cfg(W, H, tile=(32, 32)), [M.make_cloud(x, y, value=v, time=np.float32(sign) * v)])
    got = M.bands(pipe)[0]
    m = count > 0
    assert m.any() and np.array_equal(np.isnan(got), ~m)
    assert np.array_equal(got[m].view(np.uint32), np.asarray(want, dtype=np.float32)[m].view(np.uint32))


def test_three_ingests_in_every_order():
    W, H = 33, 29
    parts = [M.tricky_cloud(W, H, 2500, seed=s, stamps="ties" if s == 2 else "mixed") for s in (1, 2, 3)]
    og = M.oracle_grid(W, H, tile=(16, 16))
    words = np.zeros(W * H, dtype=np.uint64)
    for x, y, v, t in parts:
        M.fold_words(M.cells_oracle(og, x, y), v, t, W * H, words=words)
    want = M.band_of_words(words, (H, W))
    for order in itertools.permutations(range(3)):
        pipe = run_host(M.make_cfg(W, H, tile=(16, 16), threads=3),
                        [M.make_cloud(parts[i][0], parts[i][1], value=parts[i][2], time=parts[i][3]) for i in order])
        M.assert_bits(M.bands(pipe)[0], want, f"order {order}")


def test_filter_keeps_what_the_model_keeps():
    W, H, n = 30, 30, 5000
    x, y, v, t = M.tricky_cloud(W, H, n, seed=21)
    cls = np.random.default_rng(2).integers(0, 4, n).astype(np.float32)
    cfg = M.make_cfg(W, H, tile=(16, 16), threads=2)
    f = pcr.FilterSpec()
    f.add("cls", pcr.CompareOp.GreaterEqual, 2.0)
    cfg.filter = f
    pipe = run_host(cfg, [M.make_cloud(x, y, value=v, time=t, cls=cls)])
    cell = M.cells_oracle(M.oracle_grid(W, H, tile=(16, 16)), x, y)
    M.assert_bits(M.bands(pipe)[0], M.model_band(cell, v, t, (H, W), keep=cls >= 2.0), "filtered")


def test_shares_no_group_with_the_accumulations_of_its_channel():
    """Average and Max of the same value channel beside MostRecent: their bands are those of a pipeline without it; two
    MostRecent specs with different timestamp channels are two selections."""
    W, H, n = 40, 30, 8000
    x, y, v, t = M.tricky_cloud(W, H, n, seed=4)
    t2 = -t
    cloud = M.make_cloud(x, y, value=v, time=t, time2=t2)
    both = run_host(M.make_cfg(W, H, threads=2), [cloud],
                    [M.spec(T.Average), M.most_recent_spec(), M.spec(T.Max), M.most_recent_spec(stamp="time2")])
    alone = run_host(M.make_cfg(W, H, threads=2), [cloud], [M.spec(T.Average), M.spec(T.Max)])
    b, a = M.bands(both), M.bands(alone)
    M.assert_bits(b[0], a[0], "Average")
    M.assert_bits(b[2], a[1], "Max")
    cell = M.cells_oracle(M.oracle_grid(W, H), x, y)
    M.assert_bits(b[1], M.model_band(cell, v, t, (H, W)), "MostRecent(time)")
    M.assert_bits(b[3], M.model_band(cell, v, t2, (H, W)), "MostRecent(time2)")


def test_checkpoint_layout_and_resume(tmp_path):
    """save_state writes the reference's layout -- type 8, two float planes {value, timestamp}, an empty cell
    {NaN 0x7FC00000, -FLT_MAX} -- and load_state into a fresh pipeline continues as if uninterrupted."""
    W, H = 40, 24
    x1, y1, v1, t1 = M.tricky_cloud(W, H, 1500, seed=31)
    x1 = np.clip(x1, -3, 15.5)                                      # the left tile column only
    x2, y2, v2, t2 = M.tricky_cloud(W, H, 3000, seed=32, stamps="ties")
    og = M.oracle_grid(W, H, tile=(16, 16))
    d = str(tmp_path / "ckpt")
    a = run_host(M.make_cfg(W, H, tile=(16, 16), threads=2), [M.make_cloud(x1, y1, value=v1, time=t1)])
    a.save_state(d)
    names = sorted(os.listdir(d))
    assert names == ["tile_0000_0000.pcrt", "tile_0001_0000.pcrt"], names        # single reduction: the reference's layout
    words1 = M.fold_words(M.cells_oracle(og, x1, y1), v1, t1, W * H)
    val, ts = M.state_of_words(words1, (H, W))
    row, col, st, rt = pcr.read_tile_state(os.path.join(d, "tile_0001_0000.pcrt"))
    assert (row, col) == (1, 0) and rt == T.MostRecent and st.shape == (2, 8, 16) and st.dtype == np.float32
    assert np.array_equal(st[0].view(np.uint32), val[16:24, 0:16].view(np.uint32))
    assert np.array_equal(st[1].view(np.uint32), ts[16:24, 0:16].view(np.uint32))
    empty = words1.reshape(H, W)[16:24, 0:16] == 0
    assert empty.any() and (st[0].view(np.uint32)[empty] == 0x7FC00000).all() and (st[1][empty] == -M.FLT_MAX).all()
    # header of include/pcr/io/tile_state_io.h: ..., state_floats, reduction type
    raw = open(os.path.join(d, "tile_0001_0000.pcrt"), "rb").read()
    magic, version, hrow, hcol, cols, rows, floats = struct.unpack("<4sI5i", raw[:28])
    assert (magic, version, hrow, hcol, cols, rows, floats, raw[28]) == (b"PCRT", 1, 1, 0, 16, 8, 2, 8)
    assert len(raw) == 36 + 2 * 16 * 8 * 4

    b = pcr.Pipeline.create(_with(M.make_cfg(W, H, tile=(16, 16), threads=3)))
    b.load_state(d)
    b.ingest(M.make_cloud(x2, y2, value=v2, time=t2))
    b.finalize()
    words = M.fold_words(M.cells_oracle(og, x2, y2), v2, t2, W * H, words=words1.copy())
    M.assert_bits(M.bands(b)[0], M.band_of_words(words, (H, W)), "resumed")
    # resume without further ingest: the untouched tile column stays NaN
    e = pcr.Pipeline.create(_with(M.make_cfg(W, H, tile=(16, 16))))
    e.load_state(d)
    e.finalize()
    got = M.bands(e)[0]
    M.assert_bits(got, M.band_of_words(words1, (H, W)), "loaded")
    assert np.isnan(got[:, 16:]).all()


def test_a_loaded_state_is_judged_by_the_acceptance_rule(tmp_path):
    """A file whose timestamp plane holds NaN / -inf / -FLT_MAX means empty there, whatever its value plane says."""
    W = H = 8
    st = np.zeros((2, H, W), dtype=np.float32)
    st[0] = np.arange(64, dtype=np.float32).reshape(H, W)
    st[1] = 5.0
    st[1, 0, 0], st[1, 0, 1], st[1, 0, 2], st[1, 0, 3] = np.nan, -np.inf, -M.FLT_MAX, -0.0
    d = str(tmp_path / "st")
    os.makedirs(d)
    pcr.write_tile_state(pcr.tile_state_filename(d, 0, 0), 0, 0, st, T.MostRecent)
    p = pcr.Pipeline.create(_with(M.make_cfg(W, H, tile=(8, 8))))
    p.load_state(d)
    # one newer point in a cell whose state was refused, one older point in an accepted cell
    p.ingest(M.make_cloud([0.5, 4.5], [7.5, 7.5], value=[-7.0, -9.0], time=[-1e30, 4.0]))
    p.finalize()
    got = M.bands(p)[0]
    want = st[0].copy()
    want[0, 0], want[0, 1], want[0, 2] = -7.0, np.nan, np.nan
    M.assert_bits(got, want, "loaded state")


def _with(cfg, reductions=None):
    cfg.reductions = reductions or [M.most_recent_spec()]
    return cfg


def test_create_and_ingest_errors():
    cfg = _with(M.make_cfg(8, 8), [M.most_recent_spec(stamp="")])
    assert pcr.Pipeline.create(cfg) is None
    assert pcr.pipeline_create_error() == "pipeline: MostRecent requires a timestamp_channel"

    x, y = np.array([1.5, 2.5]), np.array([1.5, 2.5])
    v = np.float32([1, 2])
    pipe = pcr.Pipeline.create(_with(M.make_cfg(8, 8)))
    with pytest.raises(RuntimeError, match="pipeline: timestamp channel not found: time"):
        pipe.ingest(M.make_cloud(x, y, value=v))
    with pytest.raises(RuntimeError, match="pipeline: value channel not found: value"):
        pipe.ingest(M.make_cloud(x, y, time=v))
    wrong = M.make_cloud(x, y, value=v)
    wrong.add_channel("time", pcr.DataType.Int32)
    with pytest.raises(RuntimeError, match="pipeline: timestamp channel must be Float32"):
        pipe.ingest(wrong)
    # nothing changed: the refused clouds left no state
    pipe.finalize()
    assert np.isnan(M.bands(pipe)[0]).all() and pipe.stats().points_processed == 0

    for glyph in (pcr.line_splat_spec("value", default_direction=0.3, default_half_length=2.0, max_radius_cells=4.0),
                  pcr.gaussian_splat_spec("value", default_sigma=1.0, max_radius_cells=3.0)):
        glyph.type, glyph.timestamp_channel = T.MostRecent, "time"
        p = pcr.Pipeline.create(_with(M.make_cfg(8, 8), [glyph]))
        assert p is not None
        with pytest.raises(RuntimeError, match="glyph splatting only supports"):
            p.ingest(M.make_cloud(x, y, value=v, time=v))

    # the reductions the reference declares and nobody implements stay refused
    for t in (T.Median, T.Percentile, T.PriorityMerge, T.Custom):
        assert pcr.Pipeline.create(_with(M.make_cfg(8, 8), [M.spec(t)])) is None
        assert pcr.pipeline_create_error() == "pipeline: unknown reduction type"


def test_cabi_state_floats_needs_no_gpu():
    L = A.lib()
    k = C.c_int(0)
    assert L.pcr_hip_state_floats(A.MOST_RECENT, C.byref(k)) == 0 and k.value == 2
    assert A.MOST_RECENT == int(T.MostRecent) == 8
    assert L.pcr_hip_abi_version() == 5
    # argument errors of the new entry points are host-side
    assert L.pcr_hip_scatter_select(None, None, None, None, None, None, 0) == 1
    assert L.pcr_hip_select_pack(None, None, None, 4, None) == 1
    assert L.pcr_hip_finalize_select(None, None, None, None, None) == 1
