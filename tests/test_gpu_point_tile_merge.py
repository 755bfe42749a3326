"""The Point tile pass's merge epilogue and the tile-height rule (scatter_binned.hip: k_tile_accum, point_bin_geom).

The fused merge settles, ahead of its loop, which cells of an LDS tile lie in a touched reference tile: one wave-uniform
answer when the reference tiles under the LDS tile are all touched or all untouched, one bit per cell otherwise.  The
existing fused-finalize tests use sixteen 256 x 256 reference tiles, whose borders coincide with LDS-tile borders; here the
reference tiles are not multiples of 128 cells, so LDS tiles straddle their borders in both directions, with most of them
untouched.  The tile height is chosen for whole rounds of CUs when a launch has few rounds; its result must not depend on it."""
import numpy as np
import pytest

import most_recent_common as M
import pcr
import pcr_oracle_py as O
from test_gpu_fullgrid_oracle import ALL6, check_point_bands, poison_device_memory
from test_gpu_most_recent import A, SelectRun, cabi_grid                      # noqa: F401  (A: the C-ABI fixture)
from test_gpu_pipeline_api import cloud_from, config_for, spec

pytestmark = pytest.mark.gpu


def patches(W, H, boxes, per_box, seed):
    """Points in a few small boxes (x0, x1, y0, y1): every reference tile away from them stays untouched."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(x0, x1, per_box) for x0, x1, _, _ in boxes])
    y = np.concatenate([rng.uniform(y0, y1, per_box) for _, _, y0, y1 in boxes])
    return x, y, rng.uniform(-1, 1, x.size).astype(np.float32)


def fused_run(og, names, x, y, v):
    poison_device_memory(8 * og.width * og.height * 4)
    p = pcr.Pipeline.create(config_for(og, [spec(t) for t in names], scatter_path=2))
    p.ingest(cloud_from(x, y, {"value": v}, "device"))
    info = p.last_scatter()
    assert info["path"] == "binned" and info["bands_with_scatter"] == 1, info
    p.finalize()
    return p, info


# Sum + Count + Average is the headline's kernel (12 B per cell); all five use all four planes (20 B per cell, a lower tile)
@pytest.mark.parametrize("names", [["Sum", "Count", "Average"], ALL6], ids=["sum_count_avg", "all_five"])
@pytest.mark.parametrize("tile", [(200, 72), (72, 200), (136, 24)], ids=lambda t: f"ref{t[0]}x{t[1]}")
def test_reference_tiles_that_straddle_lds_tiles(names, tile):
    W, H = 1000, 648                                             # 5 x 9 reference tiles of 200 x 72; 8 x 7 LDS tiles of 128 x 96
    og = O.make_grid((0, 0, W, H), tile=tile)
    # boxes that cross reference-tile borders, lie inside one tile, and sit in the last (partial) LDS column and row
    boxes = [(190, 215, 60, 80), (410, 440, 300, 330), (900, 998, 2, 40), (5, 30, 600, 646), (590, 610, 425, 440)]
    x, y, v = patches(W, H, boxes, 4000, seed=5)
    p, info = fused_run(og, names, x, y, v)
    assert tuple(info["lds_tile"])[0] == 128
    check_point_bands(p, og, x, y, v, names)                      # (exact NaN mask for every reduction)
    # a second ingest (the read-modify-write merge) on top, into other tiles as well
    x2, y2, v2 = patches(W, H, [(300, 330, 100, 130), (190, 215, 60, 80)], 3000, seed=6)
    p.ingest(cloud_from(x2, y2, {"value": v2}, "device"))
    assert p.last_scatter()["bands_with_scatter"] == 0
    p.finalize()
    check_point_bands(p, og, np.concatenate([x, x2]), np.concatenate([y, y2]), np.concatenate([v, v2]), names)


def test_more_than_64_reference_tiles_under_one_lds_tile():
    """8 x 8-cell reference tiles: 16 x 12 of them under an LDS tile, far more than a wave ballots -- the per-cell map."""
    W, H = 256, 208
    og = O.make_grid((0, 0, W, H), tile=(8, 8))
    x, y, v = patches(W, H, [(3, 60, 3, 50), (120, 135, 90, 110), (250, 255.5, 200, 207.5)], 1500, seed=8)
    rng = np.random.default_rng(9)                                # and single points all over: a checkerboard of touched tiles
    xs, ys = rng.uniform(0, W, 300), rng.uniform(0, H, 300)
    x, y, v = np.concatenate([x, xs]), np.concatenate([y, ys]), np.concatenate([v, rng.uniform(-1, 1, 300).astype(np.float32)])
    p, _ = fused_run(og, ALL6, x, y, v)
    check_point_bands(p, og, x, y, v, ALL6)


def test_all_touched_and_none_touched_lds_tiles():
    """Every reference tile under most LDS tiles touched (the uniform answer, several tiles), a corner of the grid empty."""
    W, H = 1000, 648
    og = O.make_grid((0, 0, W, H), tile=(200, 72))
    rng = np.random.default_rng(12)
    n = 400_000
    x, y = rng.uniform(0, 600, n), rng.uniform(0, H, n)           # columns 600.. untouched: two whole columns of reference tiles
    v = rng.uniform(0, 1, n).astype(np.float32)
    p, _ = fused_run(og, ["Sum", "Count", "Average"], x, y, v)
    check_point_bands(p, og, x, y, v, ["Sum", "Count", "Average"])


def geometry(W, H, names, n=20_000, seed=1):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    v = rng.uniform(0, 1, n).astype(np.float32)
    p = pcr.Pipeline.create(config_for(O.make_grid((0, 0, W, H), tile=(4096, 4096)), [spec(t) for t in names], scatter_path=2))
    p.ingest(cloud_from(x, y, {"value": v}, "device"))
    info = p.last_scatter()
    assert info["path"] == "binned", info
    return tuple(info["lds_tile"]), info["num_bins"]


def test_tile_height_rule():
    """256 CUs.  The height is today's (as many rows as fit ~150 KB, at most 128) unless a taller one that fits the
    workgroup's LDS has fewer rounds x rows, and only for launches of at most 16 rounds."""
    # C2 / point_avg: 12 B per cell, 128 x 96 -> 1 376 bins = 5.375 rounds; 128 x 104 -> 1 280 = 5 rounds
    assert geometry(4096, 4096, ["Sum", "Count", "Average"]) == ((128, 104), 1280)
    assert geometry(4096, 4096, ["Average"]) == ((128, 104), 1280)
    # C4: 8 B per cell, 128 x 128 -> 1 024 bins = 4 rounds; nothing that fits does better
    assert geometry(4096, 4096, ["Max", "Min"]) == ((128, 128), 1024)
    # fewer bins than CUs: one round whatever the height, so the shortest stays
    assert geometry(1024, 1024, ["Sum", "Count", "Average"]) == ((128, 96), 8 * 11)
    assert geometry(640, 520, ["Sum"]) == ((128, 128), 25)
    # all four planes, 20 B per cell (the sum's tile is f64): 128 x 56 (2 368 bins, 10 rounds); 128 x 64 would be 9 x 64 > 10 x 56
    # and does not fit the LDS either
    assert geometry(4096, 4096, ALL6) == ((128, 56), 32 * 74)
    # more than 16 rounds: left alone (the pinned shapes of the large-grid tests: 43 rounds, and 146.5 with four planes)
    assert geometry(16384, 8192, ["Sum", "Count"], n=200_000) == ((128, 96), 11008)
    assert geometry(16384, 16384, ["Count", "Max", "Min", "Sum"], n=200_000) == ((128, 56), 37504)


# Tiles taller than 128 rows.  256 CUs, 32 tile columns at W = 4096: 1 088 rows are nine tile rows of 128 (288 tiles, two
# rounds) or eight of 136 (256 tiles, one round) at 8 B per cell; 1 984 rows are sixteen of 128 (two rounds) or eight of 248
# (one round) at 4 B per cell -- 128 x 248 = 31 744 local cells, the most the rule can choose under the 15-bit local cell
# (256 rows never beat 128: half the tile rows are never fewer than half the rounds).
TALL = [(["Sum"], 1088, 136), (["Max", "Min"], 1088, 136), (["Count"], 1984, 248)]


@pytest.mark.parametrize("names,H,tile_h", TALL, ids=["sum_136", "max_min_136", "count_248"])
def test_point_tiles_taller_than_128_rows(names, H, tile_h):
    W = 4096
    og = O.make_grid((0, 0, W, H), tile=(1000, 500))             # reference-tile borders inside the tall LDS tiles
    rng = np.random.default_rng(21)
    n = 300_000                                                  # everywhere but a strip on the right; the last rows crowded
    x = np.concatenate([rng.uniform(0, 2900, n), rng.uniform(0, W, 20_000)])
    y = np.concatenate([rng.uniform(0, H, n), rng.uniform(H - 3, H, 20_000)])
    v = rng.uniform(-1, 1, x.size).astype(np.float32)
    p, info = fused_run(og, names, x, y, v)
    assert tuple(info["lds_tile"]) == (128, tile_h) and info["num_bins"] == 256, info
    check_point_bands(p, og, x, y, v, names)
    p.ingest(cloud_from(x[:50_000] + 1100, y[:50_000], {"value": v[:50_000]}, "device"))      # the read-modify-write merge
    p.finalize()
    check_point_bands(p, og, np.concatenate([x, x[:50_000] + 1100]), np.concatenate([y, y[:50_000]]),
                      np.concatenate([v, v[:50_000]]), names)


@pytest.mark.parametrize("fresh", [0, 2])
def test_most_recent_tiles_taller_than_128_rows(A, fresh):
    """k_tile_select on the geometry of an 8-byte cell: 128 x 136, local cells beyond 128 x 128."""
    W, H = 4096, 1088
    x, y, v, t = M.tricky_cloud(W, H, 60_000, seed=23, stamps="ties")
    cell = M.cells_oracle(M.oracle_grid(W, H, tile=(4096, 4096)), x, y)
    run = SelectRun(A, cabi_grid(A, W, H), 2, define=fresh != 2)
    try:
        run.scatter(x, y, v, t, fresh=fresh)
        st = run.stats()
        assert (st.lds_tile_w, st.lds_tile_h, st.num_bins) == (128, 136, 256)
        assert np.array_equal(run.words(), M.fold_words(cell, v, t, W * H))
    finally:
        run.close()


def test_the_tile_height_does_not_change_the_result():
    """C2's shape (128 x 104 tiles) against the direct path (no tiles at all): Count to the bit, Sum and Average to float32
    accumulation error (the direct path adds in float32, in any order: 2 M points, an eighth of a point per cell)."""
    G, n = 4096, 2_000_000
    names = ["Sum", "Count", "Average"]
    rng = np.random.default_rng(3)
    x, y = rng.uniform(2, G - 2, n), rng.uniform(2, G - 2, n)
    v = rng.uniform(0, 1, n).astype(np.float32)
    og = O.make_grid((0, 0, G, G), tile=(4096, 4096))
    got = {}
    for path in (2, 1):
        p = pcr.Pipeline.create(config_for(og, [spec(t) for t in names], scatter_path=path))
        p.ingest(cloud_from(x, y, {"value": v}, "device"))
        info = p.last_scatter()
        p.finalize()
        got[path] = [np.array(p.result().band_array(b)) for b in range(len(names))]
        if path == 2:
            assert info["path"] == "binned" and info["bands_with_scatter"] == 1 and tuple(info["lds_tile"]) == (128, 104)
        else:
            assert info["path"] == "direct"
    for name, a, b in zip(names, got[2], got[1]):
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        m = ~np.isnan(a)
        if name in ("Sum", "Average"):
            assert (np.abs(a[m].astype(np.float64) - b[m]) <= 1e-5 * np.maximum(1.0, np.abs(b[m]))).all(), name
        else:
            assert np.array_equal(a[m], b[m]), name
