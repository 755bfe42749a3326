"""Points on cell edges (tests/routing_lattice.py) on the CPU: the clouds really hold the points on which a product with
1 / cell_size floors differently from the reference's true division (so that no test of them passes vacuously), both host
world_to_cell implementations put every one of them in the reference's cell, and the host engine's Point bands are the
oracle's bit for bit."""
import numpy as np
import pytest

import pcr
import pcr_oracle_py as O

import routing_lattice as R


def test_the_clouds_hold_what_the_tests_need():
    counts = {}
    for name in R.NAMES:
        print(R.report(name))
        og = R.grid(name)
        x, y, v = R.cloud(name)
        dx, dy = R.disagreements(og, x, y)
        counts[name] = int(dx.sum()), int(dy.sum())
        assert (~R.in_bounds(og, x, y)).sum() == 4, name       # the outer neighbours of the four bounds, and nothing else
        assert len(v) == len(x) == len(y) and v.min() == 1.0 and v.max() == 7.0
    for name in ("tenth", "tenth_one_tile", "seven_tenths", "south_up"):
        assert min(counts[name]) >= 100, (name, counts[name])
    assert counts["utm"] == (0, 0)
    x, y, _ = R.cloud("tenth")
    assert R.on_column_multiple(R.grid("tenth"), x, y, 16).sum() >= 10        # reference-tile borders
    assert R.on_column_multiple(R.grid("tenth"), x, y, 128).sum() >= 1        # LDS-tile borders
    x, y, _ = R.cloud("seven_tenths")
    assert R.on_column_multiple(R.grid("seven_tenths"), x, y, 10).sum() >= 10
    # loose bounds: the quotients W and H are reached, and clamp
    og = R.grid("loose_bounds")
    x, y, _ = R.cloud("loose_bounds")
    div, _ = R.quotients(og, x, y)
    ok = R.in_bounds(og, x, y)
    assert (div[0][ok] == og.width).any() and (div[1][ok] == og.height).any()


def grid_config(og):
    g = pcr.GridConfig()
    g.bounds = pcr.BBox(og.min_x, og.min_y, og.max_x, og.max_y)
    g.cell_size_x, g.cell_size_y = og.cell_size_x, og.cell_size_y
    g.tile_width, g.tile_height = og.tile_width, og.tile_height
    g.width, g.height = og.width, og.height
    g.tiles_x, g.tiles_y = -(-og.width // og.tile_width), -(-og.height // og.tile_height)
    return g


@pytest.mark.parametrize("name", R.NAMES)
def test_world_to_cell_is_the_true_division(name):
    og = R.grid(name)
    x, y, _ = R.cloud(name)
    col, row, ok = R.cells(og, x, y)
    want = np.stack([col, row, ok], axis=1)
    want[~ok, :2] = 0
    gc = grid_config(og)
    for what, fn in (("GridConfig.world_to_cell", gc.world_to_cell), ("oracle", lambda a, b: O.world_to_cell(og, a, b))):
        got = np.array([fn(float(a), float(b)) for a, b in zip(x, y)], dtype=np.int64)
        got[got[:, 2] == 0, :2] = 0
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, f"{name}: {what} differs on {len(bad)} points, first ({x[bad[0]]!r}, {y[bad[0]]!r})"


KINDS = [("Sum", pcr.ReductionType.Sum, O.SUM), ("Count", pcr.ReductionType.Count, O.COUNT),
         ("Max", pcr.ReductionType.Max, O.MAX), ("Min", pcr.ReductionType.Min, O.MIN)]


@pytest.mark.parametrize("name", R.NAMES)
def test_host_engine_point_bands_bit_exact(name):
    og = R.grid(name)
    x, y, v = R.cloud(name)
    cfg = pcr.PipelineConfig()
    cfg.grid = grid_config(og)
    cfg.exec_mode = pcr.ExecutionMode.CPU
    specs = []
    for _, t, _ in KINDS:
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", t
        specs.append(r)
    cfg.reductions = specs
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None and pipe.engine() == "host", pcr.pipeline_create_error()
    cloud = pcr.PointCloud.create(len(x))
    cloud.set_x_array(np.array(x))
    cloud.set_y_array(np.array(y))
    cloud.add_channel("value", pcr.DataType.Float32)
    cloud.set_channel_array_f32("value", np.array(v))
    pipe.ingest(cloud)
    pipe.finalize()
    res = pipe.result()
    ref = O.Reduction(og, O.COUNT)
    ref.ingest(x, y, v)
    assert pipe.last_scatter()["points_valid"] == ref.points_valid() == int(R.in_bounds(og, x, y).sum())
    for b, (kind, _, rt) in enumerate(KINDS):
        got = np.array(res.band_array(b))
        want = O.run(og, rt, x, y, v)
        diff = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert len(diff) == 0, f"{name}/{kind}: {len(diff)} cells differ, first (row, col) {diff[0].tolist()}"
