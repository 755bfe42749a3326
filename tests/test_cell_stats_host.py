"""Per-cell stats (PipelineConfig::cell_stats) on the host engine and the C-ABI's host twin, against the model of
tests/cell_stats_common.py.  No GPU.  States are compared with np.array_equal on the integer planes, bands on uint32 views: no
tolerance anywhere but in the one scenario at the end, whose bounds are derived in cell_stats_common.check_scene.

A word on one preset state.  The state "N = 3e9, S1 ~ +-2^52, S2 near 2^63" cannot come from real points: Cauchy-Schwarz wants
S1^2 <= N * S2, and 2^104 > 3e9 * 2^64.  It is kept as written -- there D = N * S2 - S1^2 is negative and the contract's unsigned
128-bit integer holds it modulo 2^128, which twin and model must agree on bit for bit -- and a second pair with S1 ~ +-2^47
stands beside it, for which D ~ 2^94 is a true numerator with hi != 0."""
import ctypes as C

import numpy as np
import pytest

import cell_stats_common as K
from conftest import load_cabi

pcr = pytest.importorskip("pcr")

G = K.GRID
MEAN, VARIANCE, STDDEV = K.MEAN, K.VARIANCE, K.STDDEV


@pytest.fixture(scope="module")
def points():
    return K.pipeline_points()


def run(cfg, clouds, engine="host"):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == engine
    for c in clouds:
        p.ingest(K.make_cloud(pcr, c))
    return p


# ---- the twin alone, against the model, before either is trusted anywhere else ---------------------------------------------------
@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("origin,res", [(0.0, 0.01), (-2.0, 2.0 ** -6), (1500.0, 0.001)])
def test_band_twin_equals_the_model_on_preset_states(origin, res, ddof):
    A = load_cabi()
    n, s1, s2 = K.preset_states()
    model = K.bands(n, s1, s2, origin, res, ddof)
    for products in ([MEAN, VARIANCE, STDDEV], [STDDEV, VARIANCE, MEAN], [VARIANCE], [STDDEV, MEAN]):
        for got, k in zip(K.twin_bands(A, n, s1, s2, origin, res, ddof, products), products):
            K.bits_equal(got, model[k], f"twin against the model: product {k} of {products}, ddof {ddof}")
    nan = K.NAN_BITS
    assert (K.bits(model[MEAN])[0, 0], K.bits(model[STDDEV])[0, 0]) == (nan, nan)                   # N = 0
    assert not np.isnan(model[MEAN][0, 1]) and np.isnan(model[STDDEV][0, 1]) == (ddof == 1)         # N = 1
    assert model[STDDEV][0, 3] == 0.0 and model[VARIANCE][0, 3] == 0.0                              # D = 0
    assert np.isfinite(model[STDDEV][0, 7]) and model[STDDEV][0, 7] > 0                             # hi != 0
    own = K.twin_bands(A, n, s1, s2, origin, res, ddof, [STDDEV], own=(1, 2))                       # the owned rows alone
    K.bits_equal(own[0], model[STDDEV][1:2], "owned rows")


def test_band_values_by_hand():
    """Values anyone can check: the mean and spread of 1, 2, 3, 4 steps of 0.5 above 10."""
    A = load_cabi()
    n, s1, s2 = np.array([[4]], np.uint32), np.array([[10]], np.int64), np.array([[30]], np.uint64)
    mean, var, sd = K.twin_bands(A, n, s1, s2, 10.0, 0.5, 0, [MEAN, VARIANCE, STDDEV])
    assert mean[0, 0] == 11.25 and var[0, 0] == np.float32(1.25 * 0.25) and sd[0, 0] == np.float32(0.5 * np.sqrt(1.25))
    _, var1, sd1 = K.twin_bands(A, n, s1, s2, 10.0, 0.5, 1, [MEAN, VARIANCE, STDDEV])
    assert var1[0, 0] == np.float32((5.0 / 3.0) * 0.25) and sd1[0, 0] == np.float32(0.5 * np.sqrt(20.0 / 12.0))


def test_the_step_rule():
    res, origin = 2.0 ** -6, -2.0
    v = np.array([origin, origin + 0.5 * res, origin + 1.5 * res, origin + 2.5 * res, origin - 0.5 * res, origin - 1.5 * res,
                  np.inf, -np.inf, origin + K.Q * res, origin - K.Q * res, origin + 2 * K.Q * res, np.nan, -0.0], np.float32)
    q, counted = K.steps(v, origin, res)
    assert q.tolist() == [0, 0, 2, 2, 0, -2, K.Q, -K.Q, K.Q, -K.Q, K.Q, 0, 128] and counted.tolist() == [True] * 11 + [False, True]
    # ... and the host engine does the same: one point per cell of the first row
    c = dict(x=G["min_x"] + (np.arange(v.size) + 0.5) * G["cs"], y=np.full(v.size, G["max_y"] - 0.25), z=v)
    p = run(K.make_config(pcr, "cpu", [K.entry(pcr, "z", origin, res)]), [c])
    n, s1, s2 = p.cell_stats(0)
    assert n.dtype == np.uint32 and s1.dtype == np.int64 and s2.dtype == np.uint64 and n.shape == (G["H"], G["W"])
    assert n[0, :v.size].tolist() == [1] * 11 + [0, 1] and s1[0, :v.size].tolist() == q.tolist()
    assert s2[0, :v.size].tolist() == (q * q).tolist() and n[1:].sum() == 0


# ---- the pipeline list, at 1 and 4 threads ------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
def test_model_splits_order_and_a_filtered_entry(points, threads):
    p = K.scenario_model_and_splits(pcr, "cpu", lambda cfg, clouds: run(_threads(cfg, threads), clouds), points)
    assert p.host_threads() == threads


def _threads(cfg, threads):
    cfg.cpu_threads = threads
    return cfg


def test_threads_give_the_same_bits(points):
    one = run(K.make_config(pcr, "cpu", K.entries(pcr), cpu_threads=1), [points])
    four = run(K.make_config(pcr, "cpu", K.entries(pcr), cpu_threads=4), [points])
    one.finalize()
    four.finalize()
    for i in range(len(K.SPECS)):
        K.planes_equal(four.cell_stats(i), one.cell_stats(i), f"4 threads against 1: state {i}")
    for u, w in zip(K.result_bands(four)[1][2:], K.result_bands(one)[1][2:]):
        K.bits_equal(u, w, "4 threads against 1: band")


@pytest.mark.parametrize("threads", [1, 4])
def test_a_surface_channel_as_value_channel(points, threads):
    K.scenario_surface_channel(pcr, "cpu", lambda cfg, clouds: run(_threads(cfg, threads), clouds), points)


@pytest.mark.parametrize("threads", [1, 4])
def test_band_order_fill_and_terrain_on_the_mean(points, threads):
    K.scenario_band_order_fill_and_terrain(pcr, "cpu", lambda cfg, clouds: run(_threads(cfg, threads), clouds), points)


def test_ingest_file_decodes_a_channel_only_the_entry_names(tmp_path):
    K.scenario_ingest_file(pcr, "cpu", run, tmp_path)


def test_finalize_twice_with_an_ingest_in_between(points):
    n = len(points["x"])
    a, b = K.take(points, np.arange(0, n // 2)), K.take(points, np.arange(n // 2, n))
    p = run(K.make_config(pcr, "cpu", K.entries(pcr)), [a])
    p.finalize()
    K.check_against_model(p, a, what="first finalize")
    p.ingest(K.make_cloud(pcr, b))
    p.finalize()
    K.check_against_model(p, points, what="second finalize")


def test_an_empty_list_changes_nothing(points):
    with_e = run(K.make_config(pcr, "cpu", [K.entry(pcr)]), [points])
    without = run(K.make_config(pcr, "cpu", []), [points])
    with_e.finalize()
    without.finalize()
    n0, b0 = K.result_bands(without)
    n1, b1 = K.result_bands(with_e)
    assert n0 == ["z_1", "z_2"] and n1 == n0 + ["z_std"]
    for u, w in zip(b1, b0):
        K.bits_equal(u, w, "a reduction's band")
    with pytest.raises(RuntimeError, match="no cell_stats entry 0"):
        without.cell_stats(0)


def test_defaults_of_the_configuration():
    e = pcr.CellStatsConfig("hag")
    assert (e.value_channel, e.origin, e.resolution, e.ddof, list(e.products), list(e.band_names)) == ("hag", 0.0, 0.01, 0,
                                                                                                       [pcr.CellStat.StdDev], [])
    e = pcr.CellStatsConfig("hag", origin=0.0, resolution=0.01, products=[pcr.CellStat.Mean, pcr.CellStat.StdDev], ddof=0)
    assert list(e.products) == [pcr.CellStat.Mean, pcr.CellStat.StdDev]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_create_refuses_by_message():
    K.scenario_refusals(pcr, "cpu")


def test_checkpoints_are_refused(points, tmp_path):
    K.scenario_checkpoints_refused(pcr, "cpu", run, points, tmp_path)
    assert pcr.Pipeline.create(K.make_config(pcr, "cpu", [K.entry(pcr)], resume=True, state_dir=str(tmp_path))) is None
    assert "checkpoints do not carry the cell stats" in pcr.pipeline_create_error()


def test_a_bad_value_channel_leaves_no_state(points):
    p = run(K.make_config(pcr, "cpu", [K.entry(pcr, "height")]), [])
    with pytest.raises(RuntimeError, match="cell_stats value channel not found: height"):
        p.ingest(K.make_cloud(pcr, points))
    cloud = K.make_cloud(pcr, points)
    cloud.add_channel("height", pcr.DataType.Int32)
    with pytest.raises(RuntimeError, match="cell_stats value channel must be Float32"):
        p.ingest(cloud)
    assert not p.cell_stats(0)[0].any() and p.stats().points_processed == 0
    p.finalize()
    assert all(np.isnan(b).all() for b in K.result_bands(p)[1])


def test_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    g = A.make_grid((0, 0, 4, 4))
    n, s1, s2 = np.zeros((4, 4), np.uint32), np.zeros((4, 4), np.int64), np.zeros((4, 4), np.uint64)
    out = np.zeros((4, 4), np.float32)
    prods, ptrs = (C.c_int * 1)(STDDEV), (C.c_void_p * 1)(out.ctypes.data)
    bad_prod, null_out = (C.c_int * 1)(3), (C.c_void_p * 1)(None)
    for fn, extra in ((L.pcr_hip_cell_stats_bands, (None,)), (L.pcr_hip_cell_stats_bands_host, ())):
        ok = [C.byref(g), n.ctypes.data, s1.ctypes.data, s2.ctypes.data, 0.0, 0.01, 0, 1, prods, ptrs]
        for at, bad, msg in ((1, None, b"null argument"), (2, None, b"null argument"), (3, None, b"null argument"),
                             (8, None, b"null argument"), (9, None, b"null argument"),
                             (4, float("nan"), b"origin and resolution must be finite"), (5, 0.0, b"the resolution positive"),
                             (5, float("inf"), b"origin and resolution must be finite"), (6, 2, b"ddof must be 0 or 1"),
                             (7, 0, b"between 1 and 3 products"), (7, 4, b"between 1 and 3 products"),
                             (8, bad_prod, b"a product must be 0 (mean), 1 (variance) or 2 (standard deviation)"),
                             (9, null_out, b"null output band")):
            args = list(ok)
            args[at] = bad
            assert fn(*args, *extra) == 1 and msg in L.pcr_hip_last_error(), (at, bad)
    assert L.pcr_hip_scatter_cell_stats(None, n.ctypes.data, s1.ctypes.data, s2.ctypes.data, 0.0, 100.0, None, None, None, 0) == 1
    assert b"null engine" in L.pcr_hip_last_error()


# ---- the scenario that shows the point ----------------------------------------------------------------------------------------
def test_a_decimetre_of_noise_at_1500_metres():
    """The derived bounds (cell_stats_common.check_scene) hold on the host engine, and the obvious float32 form
    Sum(v^2)/N - mean^2 misses the same cells' standard deviation by more than ten times the bound: NumPy only, on the CPU."""
    def make(cfg, c):
        p = run(cfg, [c])
        p.finalize()
        return p
    c, cell, count, std64 = K.check_scene(pcr, make)
    bound = K.SCENE_RES / 2 + 1e-6
    miss = np.abs(K.naive_float32_std(c, cell, count) - std64)
    print(f"float32 Sum(v^2)/N - mean^2: max miss {miss.max():.3e}, median {np.median(miss):.3e}; ten times the bound {10 * bound:.3e}")
    assert (miss > 10 * bound).any()
