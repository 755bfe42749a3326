"""Shared by the reprojection tests: an exact Gauss-Krueger oracle in mpmath (and its recorded lattice), a numpy restatement of the UTM inverse, and
the pipeline case the engines are checked on (points near the cell centres of a UTM 18N grid, fed in lon/lat)."""
import numpy as np

WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563
K0 = 0.9996
FE = 500000.0


def utm_lon0(zone):
    return -183.0 + 6.0 * zone


# ---- exact oracle -----------------------------------------------------------------------------------------------------
INVF = {"WGS84": "298.257223563", "GRS80": "298.257222101"}   # inverse flattenings, as EPSG states them
ORACLE_DPS = 50
ORACLE_RESIDUAL = 1e-30


def _ellipsoid(mp, ellipsoid):
    a, f = mp.mpf(WGS84_A), 1 / mp.mpf(INVF[ellipsoid])
    e2 = f * (2 - f)
    return a, e2, mp.sqrt(e2)


def oracle_quarter_meridian(ellipsoid="WGS84", dps=ORACLE_DPS):
    """k0 times the meridian arc from the equator to the pole, by quadrature (an mpf)."""
    import mpmath as mp
    with mp.workdps(dps):
        a, e2, _ = _ellipsoid(mp, ellipsoid)
        return mp.mpf(K0) * mp.quad(lambda s: a * (1 - e2) * (1 - e2 * mp.sin(s) ** 2) ** mp.mpf(-1.5), [0, mp.pi / 2])


def oracle_tm(lat_deg, dlon_deg, dps=ORACLE_DPS, ellipsoid="WGS84"):
    """(x, y) of the exact Gauss-Krueger map on the ellipsoid, k0 = 0.9996, no false easting / northing: solve
    psi(phi_c) = psi(phi) + i lambda for the complex latitude phi_c, then y + i x = k0 M(phi_c), with M the meridian arc
    continued analytically.  Independent of any series.  The root search starts from the Gauss-Schreiber point (the
    answer on the sphere); the residual of the root it returns is asserted, so the start cannot influence the answer.
    |lat| = 90 exactly is the pole row: x = 0, y = +-k0 (quarter meridian)."""
    import mpmath as mp
    with mp.workdps(dps):
        if abs(lat_deg) == 90.0:
            return 0.0, float(mp.sign(lat_deg) * oracle_quarter_meridian(ellipsoid, dps))
        a, e2, e = _ellipsoid(mp, ellipsoid)

        def psi(p):
            return mp.asinh(mp.tan(p)) - e * mp.atanh(e * mp.sin(p))

        phi, lam = mp.radians(mp.mpf(lat_deg)), mp.radians(mp.mpf(dlon_deg))
        target = psi(phi) + 1j * lam
        start = mp.mpc(mp.atan2(mp.tan(phi), mp.cos(lam)), mp.atanh(mp.cos(phi) * mp.sin(lam)))
        pc = mp.findroot(lambda z: psi(z) - target, start, tol=mp.mpf(10) ** (-2 * dps), verify=False, maxsteps=100)
        residual = abs(psi(pc) - target)
        assert residual <= ORACLE_RESIDUAL, f"oracle_tm({lat_deg}, {dlon_deg}, {ellipsoid}): residual {mp.nstr(residual, 5)}"
        m = pc * mp.quad(lambda s: a * (1 - e2) * (1 - e2 * mp.sin(s * pc) ** 2) ** mp.mpf(-1.5), [0, 1])
        w = mp.mpf(K0) * m
        return float(w.imag), float(w.real)


def oracle_wm(lat_deg, lon_deg, dps=ORACLE_DPS):
    """(x, y) of Web Mercator (EPSG:3857) by its closed forms on the sphere of radius a: x = a lambda, y = a atanh(sin phi)."""
    import mpmath as mp
    with mp.workdps(dps):
        a = mp.mpf(WGS84_A)
        return float(a * mp.radians(mp.mpf(lon_deg))), float(a * mp.atanh(mp.sin(mp.radians(mp.mpf(lat_deg)))))


def oracle_utm(lat_deg, lon_deg, zone, south=False, ellipsoid="WGS84"):
    x, y = oracle_tm(lat_deg, lon_deg - utm_lon0(zone), ellipsoid=ellipsoid)
    return FE + x, y + (10000000.0 if south else 0.0)


# ---- the recorded oracle (tests/golden/make_reproject_lattice.py) -----------------------------------------------------
def eta_prime(lat_deg, dlon_deg):
    """|eta'| = atanh(cos(chi) sin|dlon|), chi the conformal latitude (WGS 84; GRS80 differs by 1e-11 relative): the
    Gauss-Schreiber easting the transform puts its cut on."""
    e = np.sqrt(WGS84_F * (2 - WGS84_F))
    phi = np.radians(np.asarray(lat_deg, float))
    psi = np.arcsinh(np.tan(phi)) - e * np.arctanh(e * np.sin(phi))
    return np.arctanh(np.sin(np.radians(np.abs(dlon_deg))) / np.cosh(psi))


def load_lattice():
    """The arrays of tests/golden/reproject_lattice.npz plus eta (the Gauss-Schreiber easting of each point) and inside
    (eta below the cut: the points the transform accepts)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject_lattice.npz"))
    L = {k: z[k] for k in z.files}
    L["eta"] = eta_prime(L["lat"], L["dlon"])
    L["inside"] = L["eta"] < float(L["eta_cut"])
    return L


def edge_inputs():
    """Exact inputs at the edges of the domain, as (lon offset from the central meridian, lat): the poles and the next
    double beyond them, either side of the cut on the equator (1e-9 relative away from it), 90 degrees - 1e-6 from the
    central meridian, and NaN / +-inf on each axis."""
    cut = np.degrees(np.arcsin(np.tanh(1.0)))
    inf, nan = np.inf, np.nan
    dl = [0.0, 7.0, 0.0, 7.0, 0.0, 0.0, cut * (1 - 1e-9), cut * (1 + 1e-9), -cut * (1 - 1e-9), -cut * (1 + 1e-9),
          90.0 - 1e-6, 90.0 - 1e-6, nan, 1.0, inf, -inf, 1.0, 1.0]
    lat = [90.0, -90.0, np.nextafter(90.0, inf), np.nextafter(-90.0, -inf), 90.5, -91.0, 0.0, 0.0, 0.0, 0.0,
           0.0, 89.0, 10.0, nan, 10.0, 10.0, inf, -inf]
    ok = [True, True, False, False, False, False, True, False, True, False, False, True] + [False] * 6
    return np.array(dl), np.array(lat), np.array(ok)


# ---- numpy restatement of the inverse (Karney 2011: beta series, then Newton on the conformal latitude) ---------------
def _third_flattening(f=WGS84_F):
    return f / (2.0 - f)


def _beta(n):
    return [
        n / 2 - 2 * n**2 / 3 + 37 * n**3 / 96 - n**4 / 360 - 81 * n**5 / 512 + 96199 * n**6 / 604800,
        n**2 / 48 + n**3 / 15 - 437 * n**4 / 1440 + 46 * n**5 / 105 - 1118711 * n**6 / 3870720,
        17 * n**3 / 480 - 37 * n**4 / 840 - 209 * n**5 / 4480 + 5569 * n**6 / 90720,
        4397 * n**4 / 161280 - 11 * n**5 / 504 - 830251 * n**6 / 7257600,
        4583 * n**5 / 161280 - 108847 * n**6 / 3991680,
        20648693 * n**6 / 638668800,
    ]


def utm_inverse_np(x, y, zone, south=False):
    """UTM (WGS 84) -> (lon, lat) in degrees, term by term (no Clenshaw), tau from tau' by Newton."""
    n = _third_flattening()
    f = WGS84_F
    e2 = f * (2 - f)
    e = np.sqrt(e2)
    A = WGS84_A / (1 + n) * (1 + n**2 / 4 + n**4 / 64 + n**6 / 256)
    xi = (np.asarray(y, float) - (10000000.0 if south else 0.0)) / (K0 * A)
    eta = (np.asarray(x, float) - FE) / (K0 * A)
    xip, etap = xi.copy(), eta.copy()
    for j, b in enumerate(_beta(n), start=1):
        xip -= b * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        etap -= b * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    taup = np.sin(xip) / np.sqrt(np.sinh(etap) ** 2 + np.cos(xip) ** 2)
    lam = np.arctan2(np.sinh(etap), np.cos(xip))
    tau = taup / (1 - e2)
    for _ in range(5):
        s1 = np.sqrt(1 + tau**2)
        sig = np.sinh(e * np.arctanh(e * tau / s1))
        taupa = tau * np.sqrt(1 + sig**2) - sig * s1
        tau = tau + (taup - taupa) * (1 + (1 - e2) * tau**2) / ((1 - e2) * s1 * np.sqrt(1 + taupa**2))
    return utm_lon0(zone) + np.degrees(lam), np.degrees(np.arctan(tau))


# ---- the pipeline case ------------------------------------------------------------------------------------------------
GRID_EPSG = 32618
WKT_4326 = ('GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563,AUTHORITY["EPSG","7030"]],'
            'AUTHORITY["EPSG","6326"]],PRIMEM["Greenwich",0],UNIT["degree",0.0174532925199433],AUTHORITY["EPSG","4326"]]')
WKT1_UTM = ('PROJCS["WGS 84 / UTM zone 18N",GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563,'
            'AUTHORITY["EPSG","7030"]],AUTHORITY["EPSG","6326"]],PRIMEM["Greenwich",0,AUTHORITY["EPSG","8901"]],'
            'UNIT["degree",0.0174532925199433,AUTHORITY["EPSG","9122"]],AUTHORITY["EPSG","4326"]],'
            'PROJECTION["Transverse_Mercator"],PARAMETER["central_meridian",-75],UNIT["metre",1,AUTHORITY["EPSG","9001"]],'
            'AXIS["Easting",EAST],AXIS["Northing",NORTH],AUTHORITY["EPSG","32618"]]')
CELL = 10.0


def grid_bounds(size):
    x0, y0 = 580000.0, 4500000.0               # 18N, around 40.6 N, 74 W
    return (x0, y0, x0 + size * CELL, y0 + size * CELL)


def cell_points(size, n, seed=7):
    """n points at cell centres +- 0.3 cell of the grid (UTM metres) and a value each: no point lies within 0.2 cell of
    an edge, so transform errors far below a millimetre cannot move one into another cell."""
    rng = np.random.default_rng(seed)
    b = grid_bounds(size)
    col = rng.integers(0, size, n)
    row = rng.integers(0, size, n)
    x = b[0] + (col + 0.5 + rng.uniform(-0.3, 0.3, n)) * CELL
    y = b[3] - (row + 0.5 + rng.uniform(-0.3, 0.3, n)) * CELL
    v = rng.uniform(0, 1, n).astype(np.float32)
    return x, y, v


def make_config(pcr, size, exec_mode, grid_crs=None, reductions=("Count", "Sum", "Average")):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(*grid_bounds(size))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = CELL, -CELL
    cfg.grid.crs = pcr.CRS.from_epsg(GRID_EPSG) if grid_crs is None else grid_crs
    cfg.grid.compute_dimensions()
    cfg.exec_mode = exec_mode
    specs = []
    for name in reductions:
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", getattr(pcr.ReductionType, name)
        specs.append(r)
    cfg.reductions = specs
    return cfg


def make_cloud(pcr, x, y, v, crs):
    c = pcr.PointCloud.create(len(x))
    c.set_x_array(x)
    c.set_y_array(y)
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", v)
    if crs is not None:
        c.set_crs(crs)
    return c


def oracle_bands(O, size, x, y, v):
    og = O.make_grid(grid_bounds(size), cell=(CELL, -CELL))
    return [O.run(og, O.COUNT, x, y, v), O.run(og, O.SUM, x, y, v), O.run(og, O.AVERAGE, x, y, v)]


def check_bands(grid, want, what=""):
    """Count exact (NaN where empty), Sum and Average within rtol 1e-5."""
    got = [np.asarray(grid.band_array(i)) for i in range(3)]
    for k, (g, w, rtol) in enumerate(zip(got, want, (0.0, 1e-5, 1e-5))):
        g = np.asarray(g, np.float32).reshape(w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what} band {k}: NaN mask differs"
        m = ~np.isnan(w)
        if rtol == 0.0:
            assert np.array_equal(g[m], w[m]), f"{what} band {k}: differs"
        else:
            np.testing.assert_allclose(g[m], w[m], rtol=rtol, atol=1e-6, err_msg=f"{what} band {k}")
