"""GPU: the reprojection kernel (pcr_hip_transform_xy) against its host twin, and Pipeline.ingest on the HIP engine -- host,
device, page-locked async and file-streamed clouds, out of core, the full C2 shape, and ingest_unrouted over two ranks --
fed lon/lat into a UTM grid, against the host engine and the oracle on the UTM coordinates."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import reproject_common as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SIZE, N = 160, 200_000


@pytest.fixture(scope="module")
def pcr():
    import pcr as p
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def O():
    import pcr_oracle_py
    return pcr_oracle_py


@pytest.fixture(scope="module")
def case(O):
    x, y, v = R.cell_points(SIZE, N)
    lon, lat = R.utm_inverse_np(x, y, 18)
    return x, y, v, lon, lat, R.oracle_bands(O, SIZE, x, y, v)


# ---- the kernel against the host path ----------------------------------------------------------------------------------
def _device_vs_host(pcr, src, dst, x, y):
    import torch
    hx, hy = pcr.transform_xy(src, dst, x, y)
    dx, dy = pcr.transform_xy(src, dst, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    dx, dy = dx.cpu().numpy(), dy.cpu().numpy()
    assert np.array_equal(np.isnan(dx), np.isnan(hx)) and np.array_equal(np.isnan(dy), np.isnan(hy))
    m = ~np.isnan(hx)
    return np.max(np.abs(dx[m] - hx[m])), np.max(np.abs(dy[m] - hy[m]))


def test_kernel_matches_the_host_path_on_a_million_points(pcr):
    rng = np.random.default_rng(11)
    n = 1_000_000
    lon = -75.0 + rng.uniform(-25.0, 25.0, n)
    lat = rng.uniform(-85.0, 85.0, n)
    lat[:1000] = rng.uniform(90.0, 95.0, 1000)                    # outside: NaN on both
    ex, ey = _device_vs_host(pcr, 4326, 32618, lon, lat)
    assert ex <= 1e-8 and ey <= 1e-8, (ex, ey)
    ux, uy = pcr.transform_xy(4326, 32618, lon[1000:], lat[1000:])
    ux, uy = ux[~np.isnan(ux)], uy[~np.isnan(ux)]
    ex, ey = _device_vs_host(pcr, 32618, 4326, ux, uy)
    assert ex <= 1e-13 and ey <= 1e-13, (ex, ey)
    ex, ey = _device_vs_host(pcr, 32617, 32618, ux, uy)
    assert ex <= 1e-8 and ey <= 1e-8, (ex, ey)
    ex, ey = _device_vs_host(pcr, 4326, 3857, lon, lat)
    assert ex <= 1e-8 and ey <= 1e-8, (ex, ey)
    wx, wy = pcr.transform_xy(4326, 3857, lon[1000:], lat[1000:])
    ex, ey = _device_vs_host(pcr, 3857, 4326, wx, wy)
    assert ex <= 1e-13 and ey <= 1e-13, (ex, ey)
    ex, ey = _device_vs_host(pcr, 3857, 32718, wx, wy)
    assert ex <= 1e-8 and ey <= 1e-8, (ex, ey)


def test_identical_codes_and_in_place_on_the_device(pcr):
    rng = np.random.default_rng(12)
    lon, lat = -75.0 + rng.uniform(-3, 3, 5000), rng.uniform(30, 50, 5000)
    c = R.make_cloud(pcr, lon, lat, np.zeros(5000, np.float32), pcr.CRS.from_epsg(4326)).to_device()
    pcr.reproject(c, pcr.CRS.from_epsg(4326))                       # the same code: bit for bit
    h = c.to_host()
    assert np.array_equal(h.x_array(), lon) and np.array_equal(h.y_array(), lat)
    pcr.reproject(c, pcr.CRS.from_epsg(32618))
    h = c.to_host()
    ex, ey = pcr.transform_xy(4326, 32618, lon, lat)
    assert c.crs().epsg == 32618
    assert np.max(np.abs(h.x_array() - ex)) <= 1e-8 and np.max(np.abs(h.y_array() - ey)) <= 1e-8


# ---- the HIP engine ----------------------------------------------------------------------------------------------------
def _run(pcr, cfg, feed):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    feed(p)
    p.finalize()
    return p


def _gpu_cfg(pcr, **kw):
    return R.make_config(pcr, SIZE, pcr.ExecutionMode.GPU, **kw)


def test_gpu_engine_host_device_async_and_file(pcr, case, tmp_path):
    x, y, v, lon, lat, want = case
    wgs = pcr.CRS.from_epsg(4326)
    host = _run(pcr, R.make_config(pcr, SIZE, pcr.ExecutionMode.CPU),
                lambda p: p.ingest(R.make_cloud(pcr, lon, lat, v, wgs))).result()
    R.check_bands(host, want, "host engine")

    def check(p, what):
        assert p.engine() == "hip"
        R.check_bands(p.result(), want, what)
        got, ref = np.asarray(p.result().band_array(0)), np.asarray(host.band_array(0))
        assert np.array_equal(got, ref, equal_nan=True), what

    cloud = R.make_cloud(pcr, lon, lat, v, wgs)
    check(_run(pcr, _gpu_cfg(pcr), lambda p: p.ingest(cloud)), "host cloud")
    assert np.array_equal(cloud.x_array(), lon) and cloud.crs().epsg == 4326       # the caller's cloud is untouched

    dev = cloud.to_device()
    check(_run(pcr, _gpu_cfg(pcr), lambda p: p.ingest(dev)), "device cloud")
    back = dev.to_host()
    assert np.array_equal(back.x_array(), lon) and np.array_equal(back.y_array(), lat) and dev.crs().epsg == 4326

    # ingest_async on page-locked chunks: the staging buffer grows between chunks while earlier ones may be in flight
    def feed_async(p):
        for a, b in ((0, 5000), (5000, 60000), (60000, N)):
            c = pcr.PointCloud.create(b - a, pcr.MemoryLocation.HostPinned)
            c.set_x_array(lon[a:b])
            c.set_y_array(lat[a:b])
            c.add_channel("value", pcr.DataType.Float32)
            c.set_channel_array_f32("value", v[a:b])
            c.set_crs(wgs)
            p.ingest_async(c)
            p.synchronize()
    check(_run(pcr, _gpu_cfg(pcr), feed_async), "ingest_async")

    path = str(tmp_path / "lonlat.pcrp")
    pcr.write_point_cloud(path, R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_wkt(R.WKT_4326)))
    check(_run(pcr, _gpu_cfg(pcr), lambda p: p.ingest_file(path, chunk_points=30_000)), "ingest_file")

    # unchanged behaviour: auto_reproject off -- the lon/lat fall outside the UTM bounds
    cfg = _gpu_cfg(pcr)
    cfg.auto_reproject = False
    off = _run(pcr, cfg, lambda p: p.ingest(cloud)).result()
    assert all(np.isnan(np.asarray(off.band_array(i))).all() for i in range(3))


def test_gpu_engine_refuses_an_unsupported_pair(pcr, case, O):
    x, y, v, lon, lat, want = case
    half = N // 2
    p = pcr.Pipeline.create(_gpu_cfg(pcr))
    p.ingest(R.make_cloud(pcr, lon[:half], lat[:half], v[:half], pcr.CRS.from_epsg(4326)).to_device())
    with pytest.raises(RuntimeError) as e:
        p.ingest(R.make_cloud(pcr, lon[half:], lat[half:], v[half:], pcr.CRS.from_epsg(2263)))
    assert "2263" in str(e.value) and "32618" in str(e.value)
    p.finalize()
    R.check_bands(p.result(), R.oracle_bands(O, SIZE, x[:half], y[:half], v[:half]), "after refusal")


def test_out_of_core(pcr, case, tmp_path):
    x, y, v, lon, lat, want = case
    cfg = _gpu_cfg(pcr)
    cfg.gpu_memory_budget = 200_000                 # 160 x 160 cells x 3 planes + bands: a few row bands
    cfg.grid.tile_width = cfg.grid.tile_height = 32
    cfg.grid.compute_dimensions()
    cfg.state_dir = str(tmp_path)
    wgs = pcr.CRS.from_epsg(4326)
    for where in ("host", "device"):
        cloud = R.make_cloud(pcr, lon, lat, v, wgs)
        if where == "device":
            cloud = cloud.to_device()
        p = _run(pcr, cfg, lambda p: p.ingest(cloud))
        assert p.out_of_core()
        R.check_bands(p.result(), want, "out of core, " + where)
        assert cloud.crs().epsg == 4326


def test_full_size_c2_shape_lonlat_equals_utm(pcr):
    """50 M points on a 4096 x 4096 grid: fed in lon/lat, the Count band is the one of the same points fed in UTM."""
    import torch
    size, n = 4096, 50_000_000
    x, y, v = R.cell_points(size, n, seed=99)
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    lon, lat = pcr.transform_xy(32618, 4326, dx, dy)               # inverse on the device
    torch.cuda.synchronize()
    del dx, dy
    cfg = R.make_config(pcr, size, pcr.ExecutionMode.GPU, reductions=("Count",))
    utm = _run(pcr, cfg, lambda p: p.ingest(R.make_cloud(pcr, x, y, v, pcr.CRS.from_epsg(32618)).to_device()))
    want = np.asarray(utm.result().band_array(0)).copy()
    del utm
    lonlat = R.make_cloud(pcr, lon.cpu().numpy(), lat.cpu().numpy(), v, pcr.CRS.from_epsg(4326)).to_device()
    del lon, lat
    got = np.asarray(_run(pcr, cfg, lambda p: p.ingest(lonlat)).result().band_array(0))
    assert np.array_equal(got, want, equal_nan=True)
    assert np.nansum(got) == n


# ---- ingest_unrouted over two ranks (the test double of RCCL of test_gpu_native_multirank.py) ----------------------------
_RANK = r"""
import os, sys, time
import numpy as np
HERE, rank, world, out_dir, mode = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
import pcr
import reproject_common as R
x, y, v = R.cell_points(96, 40000, seed=3)
lon, lat = R.utm_inverse_np(x, y, 18)
sel = np.arange(len(x)) % world == rank
cfg = R.make_config(pcr, 96, pcr.ExecutionMode.GPU)
cfg.cuda_device_id = 0
bad_code = 2263 if rank == 1 else 4326
out = {}
if mode == "native":
    ident_path = os.path.join(out_dir, "id.bin")
    if rank == 0:
        ident = pcr.NativeShardedPipeline.make_id()
        with open(ident_path + ".part", "wb") as f:
            f.write(ident)
        os.rename(ident_path + ".part", ident_path)
    else:
        t0 = time.time()
        while not os.path.exists(ident_path):
            assert time.time() - t0 < 120, "no id from rank 0"
            time.sleep(0.01)
        ident = open(ident_path, "rb").read()
    sp = pcr.NativeShardedPipeline.create(cfg, ident, rank, world, 0)
    assert sp is not None, pcr.NativeShardedPipeline.create_error()
    unrouted, finalize, result = sp.ingest_unrouted, sp.finalize, sp.result
else:
    import torch
    import torch.distributed as dist
    from pcr.distributed import ShardedPipeline
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + os.environ["PCR_TEST_PORT"], rank=rank, world_size=world)
    sp = ShardedPipeline(cfg, rank, world, device_id=0, comm="native")
    unrouted, finalize, result = sp.ingest_unrouted, sp.finalize, sp.result
mine = R.make_cloud(pcr, lon[sel], lat[sel], v[sel], pcr.CRS.from_epsg(4326))
out["received"] = np.array(unrouted(mine))
assert np.array_equal(mine.x_array(), lon[sel]) and mine.crs().epsg == 4326
# a round in which rank 1's cloud cannot be reprojected: refused on EVERY rank, nothing accumulated
try:
    unrouted(R.make_cloud(pcr, lon[sel], lat[sel], v[sel], pcr.CRS.from_epsg(bad_code)))
    out["refused"] = np.array(0)
except RuntimeError as e:
    out["refused"] = np.array(1)
    out["msg"] = np.array(str(e))
finalize()
for b in range(3):
    out[f"b{b}"] = np.array(result().band_array(b))
np.savez(os.path.join(out_dir, f"n{rank}.npz"), **out)
if mode != "native":
    sp.close()
    dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("mode", ["native", "python"])
def test_ingest_unrouted_two_ranks(pcr, O, tmp_path, mode):
    gxx = shutil.which("g++")
    if not gxx or not os.path.isdir("/opt/rocm/include/rccl"):
        pytest.skip("g++ or the RCCL headers are not available")
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    fake = str(tmp_path / "libfake_rccl.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(HERE, "native", "fake_rccl.cpp"), "-o", fake, "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    env = dict(os.environ, PCR_HIP_RCCL=fake, PCR_FAKE_RCCL_DIR=str(tmp_path), PCR_REQUIRE_GPU_ENGINE="1",
               PCR_TEST_PORT=str(port))
    world = 2
    procs = [subprocess.Popen([sys.executable, "-c", _RANK, HERE, str(r), str(world), str(tmp_path), mode], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank hung")
        outs.append((p.returncode, so, se))
    for r, (rc, so, se) in enumerate(outs):
        assert rc == 0, f"rank {r}: " + so[-1500:] + se[-3000:]
    parts = [np.load(tmp_path / f"n{r}.npz") for r in range(world)]
    x, y, v = R.cell_points(96, 40000, seed=3)
    assert sum(int(p["received"]) for p in parts) == len(x)
    assert all(int(p["refused"]) == 1 for p in parts)
    assert "2263" in str(parts[1]["msg"]) and "another rank" in str(parts[0]["msg"])

    class Stacked:
        def band_array(self, b):
            return np.vstack([p[f"b{b}"] for p in parts])
    R.check_bands(Stacked(), R.oracle_bands(O, 96, x, y, v), "ingest_unrouted, " + mode)
