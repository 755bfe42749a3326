"""GPU: the reprojection kernel (pcr_hip_transform_xy) against the recorded exact oracle and its host twin, and
Pipeline.ingest on the HIP engine -- host, device, page-locked async and file-streamed clouds, out of core, the full C2
shape, and ingest_unrouted over two ranks -- fed lon/lat into a UTM grid, against the host engine and the oracle on the UTM
coordinates; the same from UTM into lon/lat, Web Mercator and the neighbouring zone, and with points outside the domain
mixed in."""
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


# ---- the kernel against the recorded oracle (tests/golden/reproject_lattice.npz; no mpmath here) -------------------------
@pytest.fixture(scope="module")
def lattice():
    return R.load_lattice()


def _dev(pcr, src, dst, x, y):
    import torch
    dx, dy = pcr.transform_xy(src, dst, torch.from_numpy(np.ascontiguousarray(x)).cuda(),
                              torch.from_numpy(np.ascontiguousarray(y)).cuda())
    torch.cuda.synchronize()
    return dx.cpu().numpy(), dy.cpu().numpy()


def _pair_cases(L):
    """name -> (src, dst, in x, in y, want x, want y, unit): inputs are the oracle's coordinates in the source CRS, expected
    values the oracle's in the destination; unit "m" pins 1e-6 m, "deg" 1e-10 degrees (longitude scaled by cos lat),
    "wm" Web Mercator's own pins."""
    ins, lat, dl = L["inside"], L["lat"], L["dlon"]
    FE = R.FE
    tm, nx, wm = L["tm_wgs84"], L["tm_wgs84_next"], L["wm"]
    lon3 = 3.0 + dl
    both = ins & ~np.isnan(nx[:, 0])
    w = ~np.isnan(wm[:, 0])
    wi = w & ins
    wl = wi & (np.abs(lat) <= 85.0)
    g = L["tm_grs80"]
    return {
        "G->TM": (4326, 32631, lon3[ins], lat[ins], FE + tm[ins, 0], tm[ins, 1], "m"),
        "G->TM south": (4326, 32731, lon3[ins], lat[ins], FE + tm[ins, 0], 1e7 + tm[ins, 1], "m"),
        "G->TM GRS80": (4269, 26918, -75.0 + dl[ins], lat[ins], FE + g[ins, 0], g[ins, 1], "m"),
        "TM->G": (32631, 4326, FE + tm[ins, 0], tm[ins, 1], lon3[ins], lat[ins], "deg"),
        "TM->TM 17->18": (32617, 32618, FE + tm[both, 0], tm[both, 1], FE + nx[both, 0], nx[both, 1], "m"),
        "TM->TM 60->1": (32660, 32601, FE + tm[both, 0], tm[both, 1], FE + nx[both, 0], nx[both, 1], "m"),
        "G->WM": (4326, 3857, lon3[w], lat[w], wm[w, 0], wm[w, 1], "wm"),
        "WM->G": (3857, 4326, wm[w, 0], wm[w, 1], lon3[w], lat[w], "deg11"),
        "WM->TM": (3857, 32631, wm[wi, 0], wm[wi, 1], FE + tm[wi, 0], tm[wi, 1], "m"),
        # (to |lat| <= 85: beyond, y amplifies the inverse's 1e-16 rad by a / cos lat; the pin is the one of the CPU chains)
        "TM->WM": (32631, 3857, FE + tm[wl, 0], tm[wl, 1], wm[wl, 0], wm[wl, 1], "m"),
        "G->G": (4326, 4258, lon3, np.clip(lat, -90, 90), lon3, np.clip(lat, -90, 90), "same"),
    }


WM_Y_RTOL = 1.4e-12          # as tests/test_reproject_math.py


def test_kernel_against_the_recorded_oracle(pcr, lattice):
    report = {}
    failures = []
    for name, (src, dst, x, y, wx, wy, unit) in _pair_cases(lattice).items():
        assert len(x) >= 500, name
        gx, gy = _dev(pcr, src, dst, x, y)
        if unit == "same":
            assert gx.tobytes() == wx.tobytes() and gy.tobytes() == wy.tobytes(), name
            continue
        assert not np.isnan(gx).any() and not np.isnan(gy).any(), name + ": an accepted point became NaN"
        if unit == "m":
            ex, ey, pin = np.abs(gx - wx).max(), np.abs(gy - wy).max(), (1e-6, 1e-6)
        elif unit in ("deg", "deg11"):
            ex, ey = (np.abs(gx - wx) * np.cos(np.radians(wy))).max(), np.abs(gy - wy).max()
            pin = (1e-10, 1e-10) if unit == "deg" else (1e-11, 1e-11)
        else:
            low = np.abs(wy) <= 19971868.88                          # y of latitude 85
            ex, ey, pin = np.abs(gx - wx).max(), np.abs(gy - wy)[low].max(), (1e-8, 1e-7)
            rel = np.abs(gy[~low] / wy[~low] - 1.0).max()
            report[name + " rel y > 85"] = rel
            if rel > WM_Y_RTOL:
                failures.append((name, "rel", rel))
        report[name] = (ex, ey)
        if ex > pin[0] or ey > pin[1]:
            failures.append((name, ex, ey, pin))
    print("device maxima against the oracle:", report)
    assert not failures, (failures, report)


def test_nan_mask_matches_the_host_twin(pcr, lattice):
    # the lattice keeps 1e-6 (relative) from the cut and the edge inputs 1e-9, far more than one ulp of difference between
    # the device's libm and the host's can move eta': the two masks must be equal bit for bit
    L = lattice
    el, ea, _ = R.edge_inputs()
    dl, lat = np.concatenate([L["dlon"], el, [90.0 - 1e-6, -(90.0 - 1e-6)]]), np.concatenate([L["lat"], ea, [1e-6, 30.0]])
    hx, hy = pcr.transform_xy(4326, 32631, 3.0 + dl, lat)
    fin = np.isfinite(hx)
    bad = np.array([np.nan, np.inf, -np.inf, 2e7, 5e5, 5e5, 1e300])
    bady = np.array([1.0, 1.0, np.nan, 0.0, 1.2e7, np.inf, 1.0])
    sets = {(4326, 32631): (3.0 + dl, lat), (4326, 32601): (-177.0 + dl, lat), (4326, 3857): (3.0 + dl, lat),
            (4326, 4269): (3.0 + dl, lat),
            (32631, 4326): (np.concatenate([hx[fin], bad]), np.concatenate([hy[fin], bady])),
            (32631, 32632): (np.concatenate([hx[fin], bad]), np.concatenate([hy[fin], bady])),
            (32631, 3857): (np.concatenate([hx[fin], bad]), np.concatenate([hy[fin], bady])),
            (3857, 4326): (bad, bady), (3857, 32631): (np.concatenate([bad, [4e5]]), np.concatenate([bady, [5e6]]))}
    for (src, dst), (x, y) in sets.items():
        hx2, hy2 = pcr.transform_xy(src, dst, x, y)
        gx, gy = _dev(pcr, src, dst, x, y)
        assert np.array_equal(np.isnan(hx2), np.isnan(hy2)) and np.array_equal(np.isnan(gx), np.isnan(gy)), (src, dst)
        assert np.array_equal(np.isnan(gx), np.isnan(hx2)), (src, dst, np.flatnonzero(np.isnan(gx) != np.isnan(hx2)))
        assert np.isfinite(gx[~np.isnan(gx)]).all() and np.isfinite(gy[~np.isnan(gy)]).all(), (src, dst)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_launch_shapes_offsets_in_place_and_guards(pcr, n):
    import ctypes as C
    import torch
    from pcr import _cabi as A
    lib = A.lib()
    rng = np.random.default_rng(n)
    lon, lat = -75.0 + rng.uniform(-30.0, 30.0, n), rng.uniform(-89.0, 89.0, n)
    lat[::7] = 91.0                                                  # some refused points in every block
    hx, hy = pcr.transform_xy(4326, 32618, lon, lat)
    s, d = A.CrsDesc(), A.CrsDesc()
    A.check(lib.pcr_hip_crs_from_epsg(4326, C.byref(s)))
    A.check(lib.pcr_hip_crs_from_epsg(32618, C.byref(d)))
    poison = -1.2345e300
    stream = torch.cuda.current_stream().cuda_stream
    for in_place in (False, True):
        # every array starts one element into its allocation, with a poisoned element on each side
        bufs = [torch.full((n + 2,), poison, dtype=torch.float64, device="cuda") for _ in range(4)]
        bufs[0][1:n + 1] = torch.from_numpy(lon).cuda()
        bufs[1][1:n + 1] = torch.from_numpy(lat).cuda()
        ox, oy = (bufs[0], bufs[1]) if in_place else (bufs[2], bufs[3])
        ptr = [b.data_ptr() + 8 for b in (bufs[0], bufs[1], ox, oy)]
        A.check(lib.pcr_hip_transform_xy(C.byref(s), C.byref(d), ptr[0], ptr[1], ptr[2], ptr[3], n, stream))
        torch.cuda.synchronize()
        gx, gy = ox.cpu().numpy(), oy.cpu().numpy()
        for g in (gx, gy):
            assert g[0] == poison and g[n + 1] == poison, (n, in_place)
        assert np.array_equal(np.isnan(gx[1:-1]), np.isnan(hx)) and np.array_equal(np.isnan(gy[1:-1]), np.isnan(hy))
        m = ~np.isnan(hx)
        if m.any():
            assert np.abs(gx[1:-1][m] - hx[m]).max() <= 1e-8 and np.abs(gy[1:-1][m] - hy[m]).max() <= 1e-8
        if not in_place:
            assert np.array_equal(bufs[0].cpu().numpy()[1:-1], lon) and np.array_equal(bufs[1].cpu().numpy()[1:-1], lat)


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


# ---- the directions the lon/lat -> UTM case never takes ------------------------------------------------------------------
DSIZE, DN = 96, 40_000
# destination grid -> (source code, bounds origin, cell): cells are powers of two or whole metres, so width * cell is exact
DIRECTIONS = {
    4326: (32618, (-74.0, 40.5), 2.0 ** -13),              # a UTM 18N cloud into a lon/lat grid (cells of ~10 m)
    3857: (32618, (-8237000.0, 4950000.0), 10.0),           # ... and into a Web Mercator grid
    32618: (32617, (580000.0, 4500000.0), 10.0),            # a UTM 17N cloud into the 18N grid
}


def _dir_case(pcr, O, dst):
    """Points at cell centres +- 0.3 cell of a grid in the destination CRS (as cell_points) and the oracle's bands on those
    destination coordinates; the cloud carries them in the source CRS, by the host twin -- which the CPU suite pins to the
    exact map within 1e-6 m and 1e-10 degrees, four orders below the 0.2 cell a point keeps from every edge."""
    src, (x0, y0), cell = DIRECTIONS[dst]
    bounds = (x0, y0, x0 + DSIZE * cell, y0 + DSIZE * cell)
    rng = np.random.default_rng(dst)
    col, row = rng.integers(0, DSIZE, DN), rng.integers(0, DSIZE, DN)
    x = bounds[0] + (col + 0.5 + rng.uniform(-0.3, 0.3, DN)) * cell
    y = bounds[3] - (row + 0.5 + rng.uniform(-0.3, 0.3, DN)) * cell
    v = rng.uniform(0, 1, DN).astype(np.float32)
    sx, sy = pcr.transform_xy(dst, src, x, y)
    assert np.isfinite(sx).all() and np.isfinite(sy).all()
    og = O.make_grid(bounds, cell=(cell, -cell))
    want = [O.run(og, O.COUNT, x, y, v), O.run(og, O.SUM, x, y, v), O.run(og, O.AVERAGE, x, y, v)]
    assert np.nansum(want[0]) == DN

    def cfg(mode):
        c = R.make_config(pcr, DSIZE, mode, grid_crs=pcr.CRS.from_epsg(dst))
        c.grid.bounds = pcr.BBox(*bounds)
        c.grid.cell_size_x, c.grid.cell_size_y = cell, -cell
        c.grid.compute_dimensions()
        assert (c.grid.width, c.grid.height) == (DSIZE, DSIZE)
        return c
    return src, sx, sy, v, want, cfg


@pytest.mark.parametrize("dst", sorted(DIRECTIONS))
def test_pipeline_in_the_other_directions(pcr, O, tmp_path, dst):
    src, sx, sy, v, want, cfg = _dir_case(pcr, O, dst)
    crs = pcr.CRS.from_epsg(src)
    host = _run(pcr, cfg(pcr.ExecutionMode.CPU), lambda p: p.ingest(R.make_cloud(pcr, sx, sy, v, crs))).result()
    R.check_bands(host, want, "host engine")
    ref = [np.asarray(host.band_array(i)).copy() for i in range(3)]

    def check(p, what):
        assert p.engine() == "hip"
        R.check_bands(p.result(), want, what)
        assert np.array_equal(np.asarray(p.result().band_array(0)), ref[0], equal_nan=True), what + ": Count differs from the host engine"

    ooc = cfg(pcr.ExecutionMode.GPU)
    ooc.gpu_memory_budget = 80_000                   # 96 x 96 cells x 3 planes + bands: a few row bands
    ooc.grid.tile_width = ooc.grid.tile_height = 32
    ooc.grid.compute_dimensions()
    ooc.state_dir = str(tmp_path)
    for where in ("host", "device"):
        cloud = R.make_cloud(pcr, sx, sy, v, crs)
        if where == "device":
            cloud = cloud.to_device()
        check(_run(pcr, cfg(pcr.ExecutionMode.GPU), lambda p: p.ingest(cloud)), f"{src} -> {dst}, {where} cloud")
        p = _run(pcr, ooc, lambda p: p.ingest(cloud))
        assert p.out_of_core()
        check(p, f"{src} -> {dst}, out of core, {where} cloud")
        assert cloud.crs().epsg == src


@pytest.mark.parametrize("scatter_path", [0, 1, 2])
def test_bad_points_do_not_reach_a_cell(pcr, case, scatter_path):
    x, y, v, lon, lat, want = case
    rng = np.random.default_rng(13)
    k = 60
    inf, nan = np.inf, np.nan
    blon = np.concatenate([-75.0 + rng.uniform(55.0, 89.9, k) * rng.choice([-1.0, 1.0], k),     # beyond the cut
                           rng.uniform(-76.0, -74.0, k), rng.uniform(-76.0, -74.0, k),          # |lat| > 90
                           np.full(k, nan), lon[:k], np.full(k, inf), np.full(k, -inf), lon[:k], lon[:k]])
    blat = np.concatenate([rng.uniform(-30.0, 30.0, k), rng.uniform(90.0001, 400.0, k), rng.uniform(-400.0, -90.0001, k),
                           lat[:k], np.full(k, nan), lat[:k], lat[:k], np.full(k, inf), np.full(k, -inf)])
    hx, hy = pcr.transform_xy(4326, R.GRID_EPSG, blon, blat)
    assert np.isnan(hx).all() and np.isnan(hy).all()
    order = rng.permutation(N + len(blon))                          # the bad points spread through the cloud
    alon, alat = np.concatenate([lon, blon])[order], np.concatenate([lat, blat])[order]
    av = np.concatenate([v, np.ones(len(blon), np.float32)])[order]
    cfg = _gpu_cfg(pcr)
    cfg.scatter_path = scatter_path
    for where in ("host", "device"):
        cloud = R.make_cloud(pcr, alon, alat, av, pcr.CRS.from_epsg(4326))
        if where == "device":
            cloud = cloud.to_device()
        p = _run(pcr, cfg, lambda p: p.ingest(cloud))
        assert p.engine() == "hip"
        R.check_bands(p.result(), want, f"path {scatter_path}, {where} cloud")


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
