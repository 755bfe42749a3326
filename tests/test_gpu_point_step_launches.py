"""The Point step without its small launches: the bin counts and the valid-point counters are left zeroed by the scan
instead of being zeroed ahead of the count pass, the conditional identity fill rides with the scatter pass, and the blocking
finalize reads on the host whether the scatter stored the bands.

All of that is state carried from one scatter to the next (per engine) or decided on the host, so what is checked is
repetition and interleaving: several clouds into one pipeline against the same clouds into fresh pipelines, two pipelines
of one device taking turns, the split-bin case into undefined planes, finalize in every order.  Results only -- bands
against the oracle to the tolerances of the other Point tests, `points_valid` exact -- so every case holds before and
after the change; the launch list itself is read off a kernel trace (profiles/point_step_launches.md)."""
import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
import most_recent_common as M
from test_gpu_finalize_with_scatter import OnHost
from test_gpu_fullgrid_oracle import ALL6, check_point_bands, poison_device_memory
from test_gpu_pipeline_api import cloud_from, config_for, spec

pytestmark = pytest.mark.gpu

W, H = 640, 520                      # 5 LDS-tile columns, 10 rows of them with all four planes: more than six bins
MODES = {
    "one_level": {},
    "two_level": {"PCR_HIP_DEBUG_MAX_BINS": "6", "PCR_HIP_DEBUG_TWO_LEVEL": "1"},
    "row_bands": {"PCR_HIP_DEBUG_MAX_BINS": "6", "PCR_HIP_DEBUG_TWO_LEVEL": "0"},
}


def set_mode(monkeypatch, mode):
    for k, val in MODES[mode].items():                               # read by pcr_hip_engine_create
        monkeypatch.setenv(k, val)


def grid():
    return O.make_grid((0, 0, W, H), tile=(256, 256))


def three_clouds(seed):
    """Different sizes, different tiles, points outside the grid in two of them; `cls` feeds the filter cases."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (n, (x0, x1, y0, y1)) in enumerate([(70_001, (-30, W + 30, -30, H + 30)),        # the whole grid and a rim outside
                                               (41_000, (300, 420, 100, 260)),              # a few LDS tiles
                                               (55_555, (W - 90, W + 40, -50, 200))]):      # a corner, a third of it outside
        x, y = rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)
        v = rng.uniform(-2, 2, n).astype(np.float32)
        cls = rng.integers(0, 4, n).astype(np.float32)
        out.append((x, y, v, cls))
    return out


def joined(clouds, keep_cls=None):
    x, y, v, cls = (np.concatenate([c[i] for c in clouds]) for i in range(4))
    if keep_cls is not None:
        m = cls >= keep_cls
        x, y, v = x[m], y[m], v[m]
    return x, y, v


def valid_points(og, x, y, v):
    return int(np.nansum(O.run(og, O.COUNT, x, y, v)))


def make_pipeline(og, filtered=False, **kw):
    if filtered:
        f = pcr.FilterSpec()
        f.add("cls", pcr.CompareOp.GreaterEqual, 2.0)
        kw["filter"] = f
    p = pcr.Pipeline.create(config_for(og, [spec(t) for t in ALL6], scatter_path=2, **kw))
    assert p is not None, pcr.pipeline_create_error()
    return p


def ingest(p, c):
    p.ingest(cloud_from(c[0], c[1], {"value": c[2], "cls": c[3]}, "device"))
    assert p.last_scatter()["path"] == "binned"


def check(p, og, clouds, filtered, what):
    x, y, v = joined(clouds, 2.0 if filtered else None)
    check_point_bands(OnHost(p), og, x, y, v, ALL6)
    lx, ly, lv = joined(clouds[-1:], 2.0 if filtered else None)
    assert p.last_scatter()["points_valid"] == valid_points(og, lx, ly, lv), what


@pytest.mark.parametrize("filtered", [False, True], ids=["all_points", "filter"])
@pytest.mark.parametrize("mode", list(MODES))
def test_three_clouds_into_one_pipeline_and_into_three(monkeypatch, mode, filtered):
    """What a scatter leaves behind for the next one of the same engine (zeroed counts and counters) must be as good as a
    fresh engine's: the second and third ingest of one pipeline, and the pipelines that only ever see one cloud."""
    set_mode(monkeypatch, mode)
    og = grid()
    clouds = three_clouds(3)
    poison_device_memory(6 * W * H * 4)
    one = make_pipeline(og, filtered)
    for k in range(3):
        ingest(one, clouds[k])
        one.finalize()
        check(one, og, clouds[:k + 1], filtered, f"{mode}: cloud {k} into the one pipeline")
        if k == 1:
            one.last_scatter()                                       # (stats read several times, or not at all, between scatters)
            assert one.last_scatter()["points_valid"] == valid_points(og, *joined(clouds[1:2], 2.0 if filtered else None))
    for k in range(3):
        fresh = make_pipeline(og, filtered)
        ingest(fresh, clouds[k])
        fresh.finalize()
        check(fresh, og, clouds[k:k + 1], filtered, f"{mode}: cloud {k} into a fresh pipeline")


@pytest.mark.parametrize("mode", list(MODES))
def test_two_pipelines_of_one_device_take_turns(monkeypatch, mode):
    """They share the device's scratch arena; the counts are each engine's own."""
    set_mode(monkeypatch, mode)
    og = grid()
    ca, cb = three_clouds(5), three_clouds(6)
    a, b = make_pipeline(og), make_pipeline(og)
    for k in range(3):
        ingest(a, ca[k])
        ingest(b, cb[k])
        if k != 1:                                                   # (round 1: both stay unfinalized, nothing synchronises)
            a.finalize()
            b.finalize()
            check(a, og, ca[:k + 1], False, f"{mode}: a after {k}")
            check(b, og, cb[:k + 1], False, f"{mode}: b after {k}")
        assert a.last_scatter()["points_valid"] == valid_points(og, *joined(ca[k:k + 1]))
        assert b.last_scatter()["points_valid"] == valid_points(og, *joined(cb[k:k + 1]))


def hot_spot(G, n, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(500, 510, n - 5000), rng.uniform(-10, G + 10, 5000)])      # one hot spot + a thin background
    y = np.concatenate([rng.uniform(500, 510, n - 5000), rng.uniform(-10, G + 10, 5000)])
    return x, y, rng.uniform(0, 1, n).astype(np.float32)


@pytest.mark.parametrize("location", ["device", "host"])
def test_split_bin_into_undefined_planes_with_bands_offered(location):
    """More than 2^17 points in one LDS tile, planes carved from poisoned memory, bands offered to the scatter: the planes
    get their identity values after all, the hot bin's items merge with atomics, and the finalize kernel has to run --
    in the first pipeline and in one that follows it on the same device."""
    G, n = 1024, 600_000
    og = O.make_grid((0, 0, G, G), tile=(256, 256))
    for seed in (11, 12):
        x, y, v = hot_spot(G, n, seed)
        poison_device_memory(8 * G * G * 4)
        cfg = config_for(og, [spec(t) for t in ALL6], scatter_path=2)
        cfg.result_location = pcr.MemoryLocation.Device if location == "device" else pcr.MemoryLocation.Host
        p = pcr.Pipeline.create(cfg)
        p.ingest(cloud_from(x, y, {"value": v}, "device"))
        assert p.last_scatter()["path"] == "binned"
        assert p.last_scatter()["points_valid"] == valid_points(og, x, y, v)
        p.finalize()
        check_point_bands(OnHost(p), og, x, y, v, ALL6)              # (NaN mask exact: array_equal on isnan / equal_nan)
        p.finalize()
        check_point_bands(OnHost(p), og, x, y, v, ALL6)


def test_split_bin_most_recent_into_an_undefined_plane():
    Wm = Hm = 512
    rng = np.random.default_rng(12)
    n = 400_000
    x = np.concatenate([rng.uniform(130, 250, n), rng.uniform(0, Wm, 20_000)])
    y = np.concatenate([rng.uniform(Hm - 250, Hm - 130, n), rng.uniform(0, Hm, 20_000)])
    v = rng.normal(0, 5, n + 20_000).astype(np.float32)
    t = rng.integers(0, 50, n + 20_000).astype(np.float32)
    og = M.oracle_grid(Wm, Hm, tile=(128, 128))
    want = M.model_band(M.cells_oracle(og, x, y), v, t, (Hm, Wm))
    for _ in range(2):
        poison_device_memory(4 * Wm * Hm * 8)
        cfg = M.make_cfg(Wm, Hm, tile=(128, 128), mode=pcr.ExecutionMode.GPU)
        cfg.reductions = [M.most_recent_spec()]
        cfg.scatter_path = 2
        p = pcr.Pipeline.create(cfg)
        assert p is not None, pcr.pipeline_create_error()
        p.ingest(M.make_cloud(x, y, value=v, time=t).to_device())
        assert p.last_scatter()["path"] == "binned" and p.last_scatter()["points_valid"] == n + 20_000
        p.finalize()
        M.assert_bits(M.bands(p)[0], want, "hot spot, undefined plane")


@pytest.mark.parametrize("location", ["device", "host"])
@pytest.mark.parametrize("mode", ["one_level", "two_level"])
def test_finalize_in_every_order(monkeypatch, mode, location):
    set_mode(monkeypatch, mode)
    og = grid()
    clouds = three_clouds(9)
    loc = pcr.MemoryLocation.Device if location == "device" else pcr.MemoryLocation.Host
    # twice in a row
    p = make_pipeline(og, result_location=loc)
    ingest(p, clouds[0])
    p.finalize()
    check(p, og, clouds[:1], False, "first finalize")
    p.finalize()
    check(p, og, clouds[:1], False, "second finalize")
    # ingest -> finalize -> ingest -> finalize: the second finalize has to run its kernel
    ingest(p, clouds[1])
    p.finalize()
    check(p, og, clouds[:2], False, "finalize after a second ingest")
    # finalize_async + synchronize, on a pipeline whose bands the scatter may have stored, then blocking
    q = make_pipeline(og, result_location=loc)
    ingest(q, clouds[2])
    q.finalize_async()
    q.synchronize()
    check(q, og, clouds[2:], False, "finalize_async + synchronize")
    q.finalize()
    check(q, og, clouds[2:], False, "finalize after finalize_async")
    ingest(q, clouds[0])
    q.finalize_async()
    q.synchronize()
    check(q, og, [clouds[2], clouds[0]], False, "finalize_async after a second ingest")


def test_points_valid_without_any_finalize_and_all_points_outside():
    og = grid()
    clouds = three_clouds(13)
    p = make_pipeline(og, filtered=True)
    for k in (0, 1, 2, 1):
        ingest(p, clouds[k])
        assert p.last_scatter()["points_valid"] == valid_points(og, *joined(clouds[k:k + 1], 2.0))
    x, y, v, cls = clouds[0]
    far = (x + 10.0 * W, y, v, cls)                                  # every point outside the grid
    ingest(p, far)
    assert p.last_scatter()["points_valid"] == 0
    ingest(p, clouds[2])
    assert p.last_scatter()["points_valid"] == valid_points(og, *joined(clouds[2:3], 2.0))
    p.finalize()
    check_point_bands(OnHost(p), og, *joined([clouds[0], clouds[1], clouds[2], clouds[1], clouds[2]], 2.0), ALL6)
