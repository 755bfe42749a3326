"""PipelineConfig.terrain on row-block shards: a shard lacks its neighbours' rows, so the sharded pipelines take the field off
the ranks' configuration and rank 0 derives the terrain bands from the gathered grid, behind the ground filter and the fill.
The GeoTIFF rank 0 writes must hold the unsharded pipeline's bands, bit for bit -- through pcr.distributed.ShardedPipeline on
two ranks (gloo, one device) and through the C++ ShardedPipeline at world 1."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H, N, RADIUS = 128, 192, 20_000, 2


def _paths():
    for p in (HERE, os.path.join(ROOT, "pointcloud-raster_amd", "python")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _cfg(pcr, G, mode):
    import terrain_common as T
    P = pcr.TerrainProduct
    cfg = G.pipeline_cfg(W, H, mode, radius=RADIUS)
    cfg.terrain = [T.band_cfg("dtm", P.Hillshade), T.band_cfg("dtm", P.SlopeDegrees), T.band_cfg("value_1", P.Roughness, "top roughness"),
                   T.band_cfg("hag", P.TRI, compute_edges=True)]
    cfg.grid.tile_width = cfg.grid.tile_height = 64
    cfg.grid.compute_dimensions()
    return cfg


def _worker(rank, world, port, out_dir):
    import torch                                   # before pcr: one shared HIP runtime
    import torch.distributed as dist
    _paths()
    import ground_filter_common as G
    import pcr
    from pcr.distributed import ShardedPipeline
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = _cfg(pcr, G, pcr.ExecutionMode.GPU)
        cfg.output_path = os.path.join(out_dir, "whole.tif")
        sp = ShardedPipeline(cfg, rank, world, device_id=0)
        assert sp.pipe.engine() == "hip"
        sp.ingest(G.cloud(W, H, N, seed=91).to_device())
        sp.finalize()
        res = sp.result()
        assert res.num_bands() == 3 and res.rows() == H // world          # a rank's own result: its rows of the reductions' bands
        sp.close()
        bad = _cfg(pcr, G, pcr.ExecutionMode.GPU)
        entry = pcr.TerrainBandConfig(bad.terrain[0])
        entry.source_band = "nope"
        bad.terrain = [entry]
        try:
            ShardedPipeline(bad, rank, world, device_id=0)
            raise SystemExit("a source_band that names no band was accepted")
        except RuntimeError as exc:
            assert "terrain[0].source_band 'nope' names no band of the result" in str(exc)
    finally:
        dist.destroy_process_group()


def _unsharded():
    _paths()
    import ground_filter_common as G
    import pcr
    pipe = pcr.Pipeline.create(_cfg(pcr, G, pcr.ExecutionMode.CPU))
    assert pipe is not None, pcr.pipeline_create_error()
    pipe.ingest(G.cloud(W, H, N, seed=91))
    pipe.finalize()
    return pcr, G.grid_bands(pipe.result())


def _check_file(path):
    import overviews_common as M
    pcr, want = _unsharded()
    assert pcr.read_geotiff_band_names(path) == ["value_2", "value_1", "value_5", "dtm", "hag", "dtm_hillshade", "dtm_slope",
                                                 "top roughness", "hag_tri"]
    assert len(want) == 9 and np.isnan(want[5]).any() and not np.isnan(want[5]).all()
    for b in range(9):
        M.bits_equal(pcr.read_geotiff_band(path, b), want[b], f"band {b}")


def test_two_ranks_rank_zero_derives_the_terrain_bands(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    _check_file(str(tmp_path / "whole.tif"))


_NATIVE_WORLD_ONE = r"""
import os, sys
HERE = sys.argv[1]
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "pointcloud-raster_amd", "python")):
    sys.path.insert(0, p)
import pcr
import ground_filter_common as G
import test_gpu_terrain_sharded as T
cfg = T._cfg(pcr, G, pcr.ExecutionMode.GPU)
cfg.output_path = os.path.join(sys.argv[2], "one.tif")
ident = pcr.NativeShardedPipeline.make_id()
sp = pcr.NativeShardedPipeline.create(cfg, ident, 0, 1, 0)
assert sp is not None, pcr.NativeShardedPipeline.create_error()
sp.ingest(G.cloud(T.W, T.H, T.N, seed=91).to_device())
sp.finalize()
assert sp.result().num_bands() == 3
del sp
entry = pcr.TerrainBandConfig(cfg.terrain[0])
entry.band_name = "value_1"
cfg.terrain = [entry]
assert pcr.NativeShardedPipeline.create(cfg, ident, 0, 1, 0) is None
assert "terrain[0].band_name 'value_1' clashes with another band" in pcr.NativeShardedPipeline.create_error()
print("native sharded terrain ok")
"""


def test_native_sharded_pipeline_world_one(tmp_path):
    out = subprocess.run([sys.executable, "-c", _NATIVE_WORLD_ONE, HERE, str(tmp_path)], capture_output=True, text=True, timeout=240,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "native sharded terrain ok" in out.stdout
    _check_file(str(tmp_path / "one.tif"))
