"""CPU: the coordinate transform of pcr.transform_xy (host form: pcr_hip_transform_xy_host, the same source as the kernel)
against an exact Gauss-Krueger oracle in mpmath, the closed forms of Web Mercator, chains of CRSs, the domain, identical
codes, WKT identification and refusals."""
import math

import numpy as np
import pytest

import reproject_common as R

pcr = pytest.importorskip("pcr")
mp = pytest.importorskip("mpmath")


def tr(src, dst, x, y):
    return pcr.transform_xy(src, dst, np.asarray(x, float), np.asarray(y, float))


def test_oracle_known_values():
    # two values of the exact map (30 digits), as stated with the feature
    x, y = R.oracle_tm(45.0, 3.0)
    assert abs(x - 236446.026101) < 1e-6 and abs(y - 4987329.504699) < 1e-6
    x, y = R.oracle_tm(0.0, 3.0)
    assert abs(x - 333978.556919) < 1e-6 and abs(y) < 1e-9


def _oracle_points():
    rng = np.random.default_rng(2011)
    lat = np.concatenate([[0.0, 45.0, -33.0, 84.0, -80.0, 60.0], rng.uniform(-80.0, 84.0, 194)])
    dl = np.concatenate([[3.0, 3.0, 20.0, -20.0, 15.0, -0.0], rng.uniform(-20.0, 20.0, 194)])
    return lat, dl


def test_forward_against_exact_oracle():
    lat, dl = _oracle_points()
    zone = 31                                                   # lon0 = 3
    north, south = lat >= 0, lat < 0
    worst = 0.0
    for code, sel, is_south in ((32631, north, False), (32731, south, True)):
        x, y = tr(4326, code, 3.0 + dl[sel], lat[sel])
        for la, d, gx, gy in zip(lat[sel], dl[sel], x, y):
            ex, ey = R.oracle_utm(la, 3.0 + d, zone, is_south)
            worst = max(worst, abs(gx - ex), abs(gy - ey))
    assert worst <= 1e-6, worst


def test_inverse_round_trip():
    lat, dl = _oracle_points()
    lon = 3.0 + dl
    x, y = tr(4326, 32631, lon, lat)
    lon2, lat2 = tr(32631, 4326, x, y)
    assert np.max(np.abs(lon2 - lon)) <= 1e-10 and np.max(np.abs(lat2 - lat)) <= 1e-10
    x2, y2 = tr(4326, 32631, lon2, lat2)
    assert np.max(np.abs(x2 - x)) <= 1e-6 and np.max(np.abs(y2 - y)) <= 1e-6


def test_numpy_restatement_of_the_inverse_against_the_oracle():
    # what the pipeline tests feed the engines: UTM metres -> lon/lat by tests/reproject_common.py
    rng = np.random.default_rng(5)
    lat = rng.uniform(-70.0, 80.0, 24)
    lon = -75.0 + rng.uniform(-8.0, 8.0, 24)
    ex = np.array([R.oracle_utm(a, o, 18)[0] for a, o in zip(lat, lon)])
    ey = np.array([R.oracle_utm(a, o, 18)[1] for a, o in zip(lat, lon)])
    lon2, lat2 = R.utm_inverse_np(ex, ey, 18)
    assert np.max(np.abs(lon2 - lon)) <= 1e-10 and np.max(np.abs(lat2 - lat)) <= 1e-10


def test_web_mercator_closed_form():
    rng = np.random.default_rng(3)
    lon = rng.uniform(-180.0, 180.0, 500)
    lat = rng.uniform(-85.0, 85.0, 500)
    x, y = tr(4326, 3857, lon, lat)
    a = 6378137.0
    np.testing.assert_allclose(x, a * np.radians(lon), rtol=0, atol=1e-8)
    np.testing.assert_allclose(y, a * np.log(np.tan(np.pi / 4 + np.radians(lat) / 2)), rtol=0, atol=1e-7)
    lon2, lat2 = tr(3857, 4326, x, y)
    assert np.max(np.abs(lon2 - lon)) <= 1e-11 and np.max(np.abs(lat2 - lat)) <= 1e-11


def test_chains_through_web_mercator_and_geographic():
    rng = np.random.default_rng(4)
    lat = rng.uniform(-60.0, 75.0, 300)
    lon = -75.0 + rng.uniform(-10.0, 10.0, 300)
    ux, uy = tr(4326, 32618, lon, lat)
    wx, wy = tr(4326, 3857, lon, lat)
    ux2, uy2 = tr(3857, 32618, wx, wy)                        # 3857 -> UTM = 3857 -> geographic -> UTM
    assert np.max(np.abs(ux2 - ux)) <= 1e-6 and np.max(np.abs(uy2 - uy)) <= 1e-6
    wx2, wy2 = tr(32618, 3857, ux, uy)
    assert np.max(np.abs(wx2 - wx)) <= 1e-6 and np.max(np.abs(wy2 - wy)) <= 1e-6
    # the three geographic codes are one datum: coordinates pass unchanged
    gx, gy = tr(4326, 4269, lon, lat)
    assert np.array_equal(gx, lon) and np.array_equal(gy, lat)
    # NAD83 / ETRS89 UTM: GRS80, within a fraction of a millimetre of WGS 84 UTM
    nx, ny = tr(4326, 26918, lon, lat)
    assert np.max(np.abs(nx - ux)) < 1e-3 and np.max(np.abs(ny - uy)) < 1e-3


def test_zone_to_zone_against_the_oracle():
    rng = np.random.default_rng(6)
    lat = rng.uniform(25.0, 60.0, 20)
    lon = rng.uniform(-84.0, -72.0, 20)                         # across 17N / 18N
    x17 = np.array([R.oracle_utm(a, o, 17)[0] for a, o in zip(lat, lon)])
    y17 = np.array([R.oracle_utm(a, o, 17)[1] for a, o in zip(lat, lon)])
    x18, y18 = tr(32617, 32618, x17, y17)
    for a, o, gx, gy in zip(lat, lon, x18, y18):
        ex, ey = R.oracle_utm(a, o, 18)
        assert abs(gx - ex) <= 1e-6 and abs(gy - ey) <= 1e-6


def test_outside_the_domain_is_nan():
    x, y = tr(4326, 32618, [-75.0, -75.0, -75.0 + 90.0, -75.0 + 89.0, 105.0, float("nan")],
              [90.5, -91.0, 10.0, 10.0, 10.0, 10.0])
    assert np.isnan(x[[0, 1, 2, 4, 5]]).all() and np.isnan(y[[0, 1, 2, 4, 5]]).all()
    assert np.isfinite(x[3]) and np.isfinite(y[3])              # |lon - lon0| < 90: inside
    x, y = tr(4326, 3857, [0.0, 0.0, 0.0], [90.0, -90.0, 89.0])
    assert np.isnan(x[:2]).all() and np.isnan(y[:2]).all() and np.isfinite(y[2])
    x, y = tr(4326, 4258, [10.0, 10.0], [91.0, 45.0])
    assert math.isnan(x[0]) and math.isnan(y[0]) and x[1] == 10.0 and y[1] == 45.0


def test_identical_codes_are_bit_identical():
    rng = np.random.default_rng(8)
    x = rng.uniform(-1e7, 1e7, 1000)
    y = rng.uniform(-1e7, 1e7, 1000)
    x[3] = float("nan")
    for code in (4326, 3857, 32618, 25832):
        ox, oy = tr(code, code, x, y)
        assert ox.tobytes() == x.tobytes() and oy.tobytes() == y.tobytes()


def test_in_place_reproject_of_a_host_cloud():
    lon, lat = np.array([-75.0, -74.5]), np.array([40.0, 41.0])
    c = pcr.PointCloud.create(2)
    c.set_x_array(lon)
    c.set_y_array(lat)
    c.set_crs(pcr.CRS.from_epsg(4326))
    pcr.reproject(c, pcr.CRS.from_epsg(32618))
    ex, ey = tr(4326, 32618, lon, lat)
    assert np.array_equal(c.x_array(), ex) and np.array_equal(c.y_array(), ey)
    assert c.crs().epsg == 32618


WKT1_UTM = R.WKT1_UTM
WKT2_UTM = ('PROJCRS["WGS 84 / UTM zone 18N",BASEGEOGCRS["WGS 84",DATUM["World Geodetic System 1984",'
            'ELLIPSOID["WGS 84",6378137,298.257223563,LENGTHUNIT["metre",1]]],ID["EPSG",4326]],'
            'CONVERSION["UTM zone 18N",METHOD["Transverse Mercator",ID["EPSG",9807]]],'
            'CS[Cartesian,2],USAGE[SCOPE["a ""quoted"" scope"],AREA["World"]],ID["EPSG",32618]]')
WKT_NESTED_ONLY = ('PROJCS["local",GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563]],'
                   'AUTHORITY["EPSG","4326"]],PROJECTION["Transverse_Mercator"],UNIT["metre",1]]')


def test_wkt_identification():
    assert pcr.crs_epsg(pcr.CRS.from_wkt(WKT1_UTM)) == 32618
    assert pcr.crs_epsg(pcr.CRS.from_wkt(WKT2_UTM)) == 32618
    assert pcr.crs_epsg(pcr.CRS.from_wkt('GEOGCS["WGS 84",AUTHORITY["EPSG","4326"]]')) == 4326
    assert pcr.crs_epsg(pcr.CRS.from_wkt(WKT_NESTED_ONLY)) == 0           # a nested GEOGCS authority does not count
    assert pcr.crs_epsg(pcr.CRS.from_wkt('PROJCS["fixture"]')) == 0
    assert pcr.crs_epsg(pcr.CRS.from_epsg(25832)) == 25832
    assert pcr.crs_epsg(pcr.CRS()) == 0
    # identified by WKT, transformed like the code
    x, y = tr(pcr.CRS.from_wkt(WKT1_UTM), 4326, [500000.0], [4500000.0])
    ex, ey = tr(32618, 4326, [500000.0], [4500000.0])
    assert x[0] == ex[0] and y[0] == ey[0]


def test_unsupported_and_unidentified_are_refused():
    with pytest.raises(RuntimeError, match="EPSG:2263 is not supported"):
        tr(4326, 2263, [0.0], [0.0])
    with pytest.raises(RuntimeError, match="EPSG:32661"):
        tr(32661, 4326, [0.0], [0.0])
    with pytest.raises(RuntimeError, match="unidentified"):
        tr(pcr.CRS.from_wkt('PROJCS["fixture"]'), 4326, [0.0], [0.0])
    c = pcr.PointCloud.create(1)
    c.set_x_array(np.array([1.0]))
    c.set_y_array(np.array([2.0]))
    c.set_crs(pcr.CRS.from_epsg(4326))
    with pytest.raises(RuntimeError, match="2263"):
        pcr.reproject(c, pcr.CRS.from_epsg(2263))
    assert c.x_array()[0] == 1.0 and c.crs().epsg == 4326


def test_c_abi_descriptor_and_host_entry_point():
    import ctypes as C
    from pcr import _cabi as A
    L = A.lib()
    d = A.CrsDesc()
    assert L.pcr_hip_crs_from_epsg(32718, C.byref(d)) == 0
    assert d.kind == 3 and d.lon0 == -75.0 and d.fn == 10000000.0 and d.k0 == 0.9996
    assert L.pcr_hip_crs_from_epsg(2263, C.byref(d)) == 6
    assert b"2263" in L.pcr_hip_last_error()
    s, t = A.CrsDesc(), A.CrsDesc()
    A.check(L.pcr_hip_crs_from_epsg(4326, C.byref(s)))
    A.check(L.pcr_hip_crs_from_epsg(32618, C.byref(t)))
    x, y = np.array([-75.0, -74.0]), np.array([40.0, 40.0])
    A.check(L.pcr_hip_transform_xy_host(C.byref(s), C.byref(t), x.ctypes.data, y.ctypes.data, x.ctypes.data, y.ctypes.data, 2))
    ex, ey = R.oracle_utm(40.0, -74.0, 18)
    assert x[0] == 500000.0 and abs(x[1] - ex) < 1e-6 and abs(y[1] - ey) < 1e-6
