#!/usr/bin/env python3
"""Writes tests/golden/reproject_lattice.npz: the exact maps of tests/reproject_common.py (mpmath) recorded on a lattice of
geographic points, for the tests that must not import mpmath (the GPU suite).

    python tests/golden/make_reproject_lattice.py

Points are (lat, dlon): latitude and offset from the central meridian, degrees.  Per point: the Gauss-Krueger map on
WGS 84 and on GRS80 (no false easting / northing), the WGS 84 map of the same point seen from the next zone (dlon - 6, for
zone-to-zone transforms), and Web Mercator of (lon = 3 + dlon, lat).  `oracle` marks the points that carry oracle values:
every point with eta' = atanh(cos(chi) sin(dlon)) <= ORACLE_ETA_MAX (chi the conformal latitude).  Beyond that (near the equator, past 80 degrees) the
exact map approaches its branch point at 90 (1 - e) degrees, where the root search no longer converges; the code refuses
those points by a wide margin, and they serve the NaN-mask checks only.  The oracle failing on a point marked `oracle`
raises: nothing is dropped.

The lattice keeps a relative distance of at least EDGE from the cut kTmEtaMax of csrc/reproject.hpp (ETA_CUT here; a test
compares the two), so that one ulp of difference between two libms cannot flip a point across it.
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reproject_common as R  # noqa: E402

ETA_CUT = 1.0
EDGE = 1e-6
ORACLE_ETA_MAX = 2.0
WM_LON0 = 3.0
WM_LAT_MAX = 89.999
N_RANDOM = 1000
OUT = os.path.join(HERE, "reproject_lattice.npz")


eta_prime = R.eta_prime


def points():
    lat1 = [90.0, 89.999, 84.0, 80.0, 45.0, 1.0, 1e-6]
    lats = sorted(set(lat1 + [-v for v in lat1] + [0.0, 5.0, 30.0, 60.0, 89.0]))
    mags = [0.0, 1e-9, 3.0, 20.0, 35.0, 45.0, 48.0, 49.0, 50.0, 51.0, 55.0, 60.0, 70.0, 80.0, 85.0, 89.0, 89.9]
    dls = sorted(set(mags + [-v for v in mags]))
    lat, dl = [], []
    for a in lats:
        for d in dls:
            lat.append(a)
            dl.append(d)
        # either side of the cut, where this latitude reaches it
        for eta in (ETA_CUT * (1 - EDGE), ETA_CUT * (1 + EDGE), ETA_CUT * 0.99, ETA_CUT * 1.01):
            s = np.tanh(eta) * np.sin(np.radians(89.0)) / np.tanh(eta_prime(a, 89.0))     # tanh(eta) / cos(chi)
            if s < 1.0:
                for sign in (1.0, -1.0):
                    lat.append(a)
                    dl.append(sign * float(np.degrees(np.arcsin(s))))
    rng = np.random.default_rng(2026)
    ra, rd = [], []
    while len(ra) < N_RANDOM:                                   # uniform on the sphere's accepted region
        a = float(np.degrees(np.arcsin(rng.uniform(-1.0, 1.0))))
        d = float(rng.uniform(-89.9, 89.9))
        if eta_prime(a, d) <= ETA_CUT * (1 - EDGE):
            ra.append(a)
            rd.append(d)
    return np.array(lat + ra), np.array(dl + rd)


def compute(lat, dl, idx=None):
    """The recorded arrays at the points idx (all when None)."""
    n = len(lat)
    idx = range(n) if idx is None else idx
    eta = eta_prime(lat, dl)
    out = {k: np.full((n, 2), np.nan) for k in ("tm_wgs84", "tm_grs80", "tm_wgs84_next", "wm")}
    for i in idx:
        a, d = float(lat[i]), float(dl[i])
        if eta[i] <= ORACLE_ETA_MAX:
            out["tm_wgs84"][i] = R.oracle_tm(a, d, ellipsoid="WGS84")
            out["tm_grs80"][i] = R.oracle_tm(a, d, ellipsoid="GRS80")
            if abs(d - 6.0) < 89.9 and eta_prime(a, d - 6.0) <= ETA_CUT * (1 - EDGE):
                out["tm_wgs84_next"][i] = R.oracle_tm(a, d - 6.0, ellipsoid="WGS84")
        if abs(a) <= WM_LAT_MAX:
            out["wm"][i] = R.oracle_wm(a, WM_LON0 + d)
    return out


def main():
    lat, dl = points()
    eta = eta_prime(lat, dl)
    assert not np.any(np.abs(eta / ETA_CUT - 1.0) < EDGE * (1 - 1e-6)), "a lattice point sits on the cut"
    jobs = min(16, os.cpu_count() or 1)                         # the points are independent: split them over processes
    with multiprocessing.Pool(jobs) as pool:
        parts = pool.starmap(compute, [(lat, dl, range(j, len(lat), jobs)) for j in range(jobs)])
    rec = {k: np.full_like(parts[0][k], np.nan) for k in parts[0]}
    for j, part in enumerate(parts):
        for k in rec:
            rec[k][j::jobs] = part[k][j::jobs]
    np.savez_compressed(OUT, lat=lat, dlon=dl, oracle=eta <= ORACLE_ETA_MAX, eta_cut=np.float64(ETA_CUT),
                        wm_lon0=np.float64(WM_LON0), **rec)
    print(f"{OUT}: {len(lat)} points, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
