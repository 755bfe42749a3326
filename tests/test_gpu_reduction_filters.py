"""ReductionSpec.filter on the HIP engine: the cases of reduction_filters_common on both scatter paths, host against HIP bit
for bit, the layers (out of core, row-block shards, LAS), the glyphs, and the two new C-ABI entry points against NumPy and
against pcr_hip_filter_mask, the parent's kernel."""
import ctypes as C

import numpy as np
import pytest

import pcr
import reduction_filters_common as RF
from conftest import assert_band_close, load_cabi

pytestmark = pytest.mark.gpu

PATHS = pytest.mark.parametrize("path", [1, 2], ids=["direct", "binned"])


@PATHS
@pytest.mark.parametrize("n", RF.SIZES)
def test_mixed_pipeline(n, path, tmp_path):
    p = RF.check_mixed("gpu", n, tmp_path=tmp_path, scatter_path=path)
    assert p.last_scatter()["path"] == ("direct" if path == 1 else "binned")


@PATHS
@pytest.mark.parametrize("n", RF.CFG_ONLY_SIZES)
def test_a_pipeline_filter_alone(n, path):
    for preds in RF.CFG_ONLY_PREDS.values():
        for resident in ("device", "host"):
            RF.check_cfg_filter_only("gpu", n, preds, resident=resident, scatter_path=path)


def test_a_pipeline_filter_of_17_predicates():
    RF.check_cfg_filter_too_long("gpu")


@pytest.mark.parametrize("n", RF.SIZES)
def test_mixed_pipeline_host_against_hip(n):
    c = RF.make_points(n, 100 + n)
    out = {}
    for mode in ("cpu", "gpu"):
        p = RF.create(mode, RF.MIXED, [("ret", "LessEqual", 2.0)])
        p.ingest(RF.make_cloud(c, mode))
        p.finalize()
        out[mode] = RF.bands(p), p.stats().points_processed
    assert out["cpu"][1] == out["gpu"][1]
    for b, (u, w) in enumerate(zip(out["cpu"][0], out["gpu"][0])):
        RF.assert_bits(w, u, f"band {b}: HIP against host")


@PATHS
@pytest.mark.parametrize("n", RF.SIZES)
def test_all_specs_filtered_flags_come_from_the_touch_pass(n, path):
    RF.check_all_filtered("gpu", n, scatter_path=path)


@PATHS
@pytest.mark.parametrize("n", RF.SIZES)
def test_with_a_pipeline_filter_as_well(n, path):
    RF.check_with_cfg_filter("gpu", n, scatter_path=path)


@PATHS
def test_predicate_edge_cases(path):
    RF.check_predicate_edges("gpu", scatter_path=path)
    RF.check_predicate_edges("gpu", n=20000, scatter_path=path)


@PATHS
def test_against_pipelines_of_their_own(path):
    RF.check_against_own_pipelines("gpu", scatter_path=path)
    RF.check_against_own_pipelines("gpu", n=20000, scatter_path=path)


def test_refusals():
    RF.check_refusals("gpu")


def test_filtered_groups_defer_nothing_and_unfiltered_ones_still_fuse():
    c = RF.make_points(20000, 5)
    p = RF.create("gpu", RF.ALL_FILTERED[:3], scatter_path=2)
    p.ingest(RF.make_cloud(c, "gpu"))
    assert p.last_scatter()["bands_with_scatter"] == 0 and p.last_scatter()["deferred_planes"] == 0
    q = RF.create("gpu", [RF.S("Sum"), RF.S("Count")], scatter_path=2)
    q.ingest(RF.make_cloud(c, "gpu"))
    assert q.last_scatter()["bands_with_scatter"] == 1


@PATHS
def test_two_ingests_and_a_checkpoint(tmp_path, path):
    RF.check_two_ingests_and_checkpoint("gpu", tmp_path, scatter_path=path)


def test_out_of_core_row_bands(tmp_path):
    # MIXED keeps 12 planes (MostRecent: two slots) + 9 bands = 3360 B per row, 53 760 B per 16-row tile row: a 60 000 B budget
    # makes two bands of one tile row each (tests/test_gpu_out_of_core.py sets its budgets the same way)
    cfg_filt = [("ret", "LessEqual", 2.0)]
    c = RF.make_points(20000, 17)
    p = RF.create("gpu", RF.MIXED, cfg_filt, gpu_memory_budget=60000, host_cache_budget=1 << 20, state_dir=str(tmp_path))
    assert p.out_of_core()
    p.ingest(RF.make_cloud(c, "cpu"))
    p.finalize()
    model = RF.Model(RF.MIXED, cfg_filt)
    model.ingest(c)
    RF.assert_model(p, model, "out of core")
    # every spec filtered, and the LAST group's class keeps nothing in the lower band's rows: the band is parked all the same
    specs = RF.ALL_FILTERED[:2] + [RF.S("Max", filt=[("t", "Greater", 99.0)])]
    p = RF.create("gpu", specs, gpu_memory_budget=20000, host_cache_budget=1 << 20, state_dir=str(tmp_path))
    assert p.out_of_core()
    p.ingest(RF.make_cloud(c, "cpu"))
    p.finalize()
    model = RF.Model(specs)
    model.ingest(c)
    RF.assert_model(p, model, "out of core, the last class empty")


def test_two_row_block_shards_concatenate_to_the_unsharded_bands():
    c = RF.make_points(20000, 19)
    whole = RF.create("gpu", RF.MIXED)
    whole.ingest(RF.make_cloud(c, "gpu"))
    whole.finalize()
    parts = []
    for r0, r1 in ((0, 10), (10, 24)):                           # (not tile aligned)
        p = RF.create("gpu", RF.MIXED, shard_row_begin=r0, shard_row_end=r1)
        p.ingest(RF.make_cloud(c, "gpu"))
        parts.append(p)
    # a reference tile is touched if ANY shard saw a point in it: the shards' flag union, as the sharded driver does it
    A = load_cabi()
    flags = [RF.read_touched(p) for p in parts]
    union = A.DeviceBuffer.from_numpy((flags[0] | flags[1]).astype(np.uint32))
    strips = []
    for p in parts:
        p.merge_touched(union.ptr.value)
        p.finalize()
        strips.append(RF.bands(p))
    for b, w in enumerate(RF.bands(whole)):
        RF.assert_bits(np.concatenate([strips[0][b], strips[1][b]]), w, f"band {b}: the shards' strips against the unsharded band")


def test_a_las_file_with_a_spec_filter_on_classification(tmp_path):
    RF.check_las("gpu", tmp_path)


@PATHS
def test_filtered_line_groups(path):
    RF.check_line("gpu", scatter_path=path)
    RF.check_line("gpu", n=20000, scatter_path=path)


@PATHS
def test_filtered_gaussian_average_against_a_pipeline_filter(path):
    gauss = dict(kind="gauss", sigma=1.5, maxr=4.0)
    c = RF.make_points(20000, 23)
    c["a"] = np.abs(c["a"]) + np.float32(1.0)                    # (one sign: a weighted average is then well conditioned)
    p = RF.create("gpu", [RF.S("WeightedAverage", filt=RF.CLASS2, glyph=gauss), RF.S("Count")], scatter_path=path)
    own = RF.create("gpu", [RF.S("WeightedAverage", glyph=gauss)], RF.CLASS2, scatter_path=path)
    for q in (p, own):
        q.ingest(RF.make_cloud(c, "gpu"))
        q.finalize()
    # the tolerance of test_gpu_configs_c3_c4_c5.py::test_c3_full_size_gaussian_sigma4_three_paths (one Gaussian path against
    # another: the atomics' order differs between two runs as it does between two paths), NaN masks equal
    assert_band_close(RF.bands(p)[0], RF.bands(own)[0], rtol=1e-4, atol=1e-6, what="filtered Gaussian average")


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def A():
    return load_cabi()


def class_tables(A, dev):
    """8 classes over 3 channels with shared predicates: (predicate table, class words, the same as lists of predicates)."""
    table = [("cls", 0, 2.0, []), ("ret", 0, 1.0, []), ("q", 1, 5.0, []), ("cls", 6, 0.0, [1.0, 2.0, 6.0]), ("ret", 5, 2.0, []),
             ("q", 7, 0.0, [float(v) for v in range(16)]), ("q", 2, 5.0, [])]
    preds = (A.Predicate * len(table))()
    for k, (ch, op, v, vs) in enumerate(table):
        preds[k].d_channel, preds[k].op, preds[k].value, preds[k].set_size = dev[ch].ptr.value, op, v, len(vs)
        for j, s in enumerate(vs):
            preds[k].set[j] = s
    words = [0b0000001, 0b0000011, 0b0000100, 0b0001110, 0b0110000, 0b1000001, 0b0000000, 0b1111111]
    return table, preds, words


def numpy_pred(c, ch, op, v, vs):
    return RF.pred_mask(c, (ch, RF.OPS[op], vs if op >= 6 else v))


@pytest.mark.parametrize("n", RF.SIZES)
def test_filter_classes_against_numpy_and_filter_mask(A, n):
    L = A.lib()
    c = RF.make_points(n, 900 + n)
    dev = {ch: A.DeviceBuffer.from_numpy(c[ch]) for ch in ("cls", "ret", "q")}
    table, preds, words = class_tables(A, dev)
    stride = (n + 15) // 16 * 16
    masks, counts = A.DeviceBuffer(8 * stride), A.DeviceBuffer(8 * 8)
    A.check(L.pcr_hip_filter_classes(preds, len(table), (C.c_uint32 * 8)(*words), 8, n, masks.ptr, stride, counts.ptr, None))
    got = masks.to_numpy(np.uint8, (8, stride))[:, :n]
    got_counts = counts.to_numpy(np.uint64, (8,))
    one, one_count = A.DeviceBuffer(n), A.DeviceBuffer(8)
    for j, w in enumerate(words):
        members = [k for k in range(len(table)) if w >> k & 1]
        want = np.ones(n, bool)
        for k in members:
            want &= numpy_pred(c, *table[k])
        assert np.array_equal(got[j], want.astype(np.uint8)), f"class {j}: the mask differs from NumPy"
        assert int(got_counts[j]) == int(want.sum()), f"class {j}: the count differs"
        alone = (A.Predicate * max(len(members), 1))(*[preds[k] for k in members])
        A.check(L.pcr_hip_filter_mask(alone, len(members), n, one.ptr, one_count.ptr, None))
        assert np.array_equal(got[j], one.to_numpy(np.uint8, (n,))), f"class {j}: the mask differs from pcr_hip_filter_mask's"
        assert int(one_count.to_numpy(np.uint64, (1,))[0]) == int(got_counts[j])


def test_filter_classes_without_counts_and_on_unaligned_arrays(A):
    L = A.lib()
    n = 1027
    c = RF.make_points(n + 1, 77)
    whole = A.DeviceBuffer.from_numpy(c["cls"])
    pred = (A.Predicate * 1)()
    pred[0].d_channel, pred[0].op, pred[0].value = whole.ptr.value + 4, 0, 2.0        # a channel 4 bytes off: one point per lane
    masks = A.DeviceBuffer(2 * 1031 + 1)
    A.check(L.pcr_hip_filter_classes(pred, 1, (C.c_uint32 * 2)(1, 0), 2, n, masks.ptr.value + 1, 1031, None, None))
    got = masks.to_numpy(np.uint8, (2 * 1031 + 1,))
    assert np.array_equal(got[1:1 + n], (c["cls"][1:] == 2.0).astype(np.uint8)) and (got[1032:1032 + n] == 1).all()


@pytest.mark.parametrize("grid", [RF.GRID, RF.ONE_TILE], ids=["six tiles", "one tile"])
@pytest.mark.parametrize("own_rows", [None, (5, 19)], ids=["whole grid", "row block"])
@pytest.mark.parametrize("n", RF.SIZES)
def test_engine_touch_sets_the_flags_of_a_point_scatter(A, n, own_rows, grid):
    L = A.lib()
    c = RF.make_points(n, 800 + n, grid, clustered=grid is RF.GRID)
    keep = A.DeviceBuffer.from_numpy((c["cls"] != 5.0).astype(np.uint8))
    g = A.make_grid((0.0, 0.0, 40.0, 24.0), tile=(grid["tw"], grid["th"]), own_rows=own_rows)
    dx, dy = A.DeviceBuffer.from_numpy(c["x"]), A.DeviceBuffer.from_numpy(c["y"])
    flags = []
    for masked in (False, True):
        run = A.ReductionRun(g, A.PLANE_WGT)                     # a second engine: pcr_hip_scatter_point under the same mask
        A.check(L.pcr_hip_engine_set_point_mask(run.engine, keep.ptr if masked else None))
        run.scatter(c["x"], c["y"], np.zeros(n, np.float32))
        eng = C.c_void_p()
        A.check(L.pcr_hip_engine_create(C.byref(eng), C.byref(g), 0, None))
        A.check(L.pcr_hip_engine_set_point_mask(eng, keep.ptr if masked else None))
        A.check(L.pcr_hip_engine_touch(eng, dx.ptr, dy.ptr, n))
        ptr, tx, ty = C.c_void_p(), C.c_int32(0), C.c_int32(0)
        A.check(L.pcr_hip_engine_tile_touched(eng, C.byref(ptr), C.byref(tx), C.byref(ty)))
        got = np.empty((ty.value, tx.value), np.uint32)
        A.check(L.pcr_hip_memcpy_d2h(got.ctypes.data, ptr, got.nbytes, None))
        A.check(L.pcr_hip_stream_synchronize(None))
        assert np.array_equal(got != 0, run.touched()[0] != 0), f"masked={masked}: touch and scatter_point set different flags"
        flags.append(got != 0)
        L.pcr_hip_engine_destroy(eng)
        run.close()
    if n >= 1027 and grid is RF.GRID and own_rows is None:
        assert flags[0][0, 1] and not flags[1][0, 1]             # tile (0, 1) holds class 5 only
