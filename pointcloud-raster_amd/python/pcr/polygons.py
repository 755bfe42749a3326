"""Polygon sets from text: WKT strings and GeoJSON files, for pcr.rasterize_polygons and Pipeline.set_zones.

Standard library and numpy only.  One input geometry becomes ONE polygon of the set: the rings of a POLYGON (the shell and its
holes) and, for a MULTIPOLYGON, the rings of all its parts -- a polygon of the set is all of its rings under the even-odd rule,
so holes and parts need no marking and ring orientation plays no part.  The closing vertex that WKT and GeoJSON repeat is
dropped (rings close implicitly).  Z and M ordinates are read and ignored."""
import json
import re

import numpy as np

from ._pcr import PolygonSet

_NUMBER = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_RING = re.compile(r"\(([^()]*)\)")
_HEAD = re.compile(r"^\s*(MULTIPOLYGON|POLYGON)\s*(?:ZM|Z|M)?\s*(EMPTY|\(.*\))\s*$", re.I | re.S)


def _ring(points):
    a = np.asarray(points, np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError("a ring must be a list of (x, y) positions")
    a = a[:, :2]
    if len(a) > 1 and (a[0] == a[-1]).all():
        a = a[:-1]
    if len(a) < 3:
        raise ValueError("a ring of fewer than 3 vertices")
    return a


def _build(polygons, values):
    """polygons: a list of lists of (n, 2) rings."""
    coords, ro, po = [], [0], [0]
    for rings in polygons:
        for r in rings:
            coords.append(r)
            ro.append(ro[-1] + len(r))
        po.append(len(ro) - 1)
    xy = np.concatenate(coords) if coords else np.zeros((0, 2), np.float64)
    return PolygonSet(xy, np.array(ro, np.int64), np.array(po, np.int64), None if values is None else np.asarray(values, np.float32))


def _wkt_rings(text):
    m = _HEAD.match(text)
    if not m:
        raise ValueError(f"from_wkt: not a POLYGON or MULTIPOLYGON: {text[:40]!r}")
    if m.group(2).upper() == "EMPTY":
        return []
    rings = []
    for body in _RING.findall(m.group(2)):
        pts = []
        for vertex in body.split(","):
            nums = vertex.split()
            if len(nums) < 2 or not all(re.fullmatch(_NUMBER, n) for n in nums):
                raise ValueError(f"from_wkt: bad vertex {vertex.strip()!r}")
            pts.append((float(nums[0]), float(nums[1])))
        rings.append(_ring(pts))
    if not rings:
        raise ValueError("from_wkt: no ring")
    return rings


def from_wkt(texts, values=None):
    """A PolygonSet from WKT strings, one polygon of the set per string (POLYGON or MULTIPOLYGON; EMPTY gives a polygon without
    rings, which labels nothing and keeps the numbering)."""
    if isinstance(texts, str):
        texts = [texts]
    return _build([_wkt_rings(t) for t in texts], values)


def read_geojson_polygons(path, value_property=None):
    """A PolygonSet from a GeoJSON file: a FeatureCollection, a Feature or a bare geometry; Polygon and MultiPolygon only
    (anything else raises ValueError).  Each feature is one polygon; value_property names a numeric property that becomes the burn
    value (default: feature number + 1).  The coordinates are taken as they are: reproject with pcr.transform_xy if the file's
    CRS is not the grid's."""
    with open(path, encoding="utf-8") as f:
        doc = json.load(f)
    kind = doc.get("type")
    if kind == "FeatureCollection":
        features = doc.get("features", [])
    elif kind == "Feature":
        features = [doc]
    else:
        features = [{"type": "Feature", "geometry": doc, "properties": {}}]
    polygons, values = [], []
    for i, feat in enumerate(features):
        geom = feat.get("geometry") or {}
        gtype, c = geom.get("type"), geom.get("coordinates", [])
        if gtype == "Polygon":
            rings = [_ring(r) for r in c]
        elif gtype == "MultiPolygon":
            rings = [_ring(r) for part in c for r in part]
        else:
            raise ValueError(f"read_geojson_polygons: feature {i} is a {gtype}, not a Polygon or MultiPolygon")
        polygons.append(rings)
        if value_property is not None:
            props = feat.get("properties") or {}
            if value_property not in props or isinstance(props[value_property], bool) or not isinstance(props[value_property], (int, float)):
                raise ValueError(f"read_geojson_polygons: feature {i} has no numeric property {value_property!r}")
            values.append(props[value_property])
    return _build(polygons, values if value_property is not None else None)


PolygonSet.from_wkt = staticmethod(from_wkt)
