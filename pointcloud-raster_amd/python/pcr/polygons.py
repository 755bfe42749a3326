"""Polygon sets from and to text: WKT strings and GeoJSON files, for pcr.rasterize_polygons and Pipeline.set_zones, and for
what pcr.polygonize and Pipeline.polygonize give.

Standard library and numpy only.  One input geometry becomes ONE polygon of the set: the rings of a POLYGON (the shell and its
holes) and, for a MULTIPOLYGON, the rings of all its parts -- a polygon of the set is all of its rings under the even-odd rule,
so holes and parts need no marking and ring orientation plays no part.  The closing vertex that WKT and GeoJSON repeat is
dropped (rings close implicitly).  Z and M ordinates are read and ignored.

The writers go the other way and have to MARK what the set leaves unmarked, since WKT and GeoJSON want shells and holes.  Per
polygon, a ring's depth is the number of the polygon's other rings that hold the midpoint of its first edge (even-odd ray rule):
even depth is a shell, odd depth a hole of the ring of depth - 1 that holds it.  Shells are written counter-clockwise and holes
clockwise in world coordinates (RFC 7946), the closing vertex repeated, coordinates with repr() -- they read back to the same
bits.  That is well defined when the rings of a polygon neither cross nor share an edge, as polygonize's never do (they may touch
at corners); for other sets it is undefined.  A polygon of one ring skips all of it."""
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


def _holders(rings):
    """Per ring, which of the others hold the midpoint of its first edge: a ray towards +x, an edge counted when it passes the
    point's y.  One sweep over all edges of the polygon per ring."""
    a = np.concatenate(rings)
    b = np.concatenate([np.roll(r, -1, axis=0) for r in rings])
    owner = np.repeat(np.arange(len(rings)), [len(r) for r in rings])
    out = []
    for i, r in enumerate(rings):
        nxt = r[1 % len(r)]
        px, py = 0.5 * (r[0, 0] + nxt[0]), 0.5 * (r[0, 1] + nxt[1])
        at = np.nonzero(((a[:, 1] > py) != (b[:, 1] > py)) & (owner != i))[0]
        xc = a[at, 0] + (py - a[at, 1]) / (b[at, 1] - a[at, 1]) * (b[at, 0] - a[at, 0])
        odd = np.bincount(owner[at][xc > px], minlength=len(rings)) % 2
        out.append(np.nonzero(odd)[0].tolist())
    return out


def _turned(ring, ccw):
    """The ring counter-clockwise (or clockwise) in world coordinates: reversed when its shoelace sum says otherwise."""
    d = ring - ring[0]                                   # (about its first vertex: no cancellation at UTM magnitudes)
    n = np.roll(d, -1, axis=0)
    area2 = float(np.sum(d[:, 0] * n[:, 1] - n[:, 0] * d[:, 1]))
    return ring if (area2 > 0) == ccw else ring[::-1]


def _parts(rings):
    """[(shell, [holes])] of one polygon's rings, wound as RFC 7946 asks."""
    if len(rings) == 1:
        return [(_turned(rings[0], True), [])]
    holders = _holders(rings)
    depth = [len(h) for h in holders]
    parts, place = [], {}
    for i, r in enumerate(rings):
        if depth[i] % 2 == 0:
            place[i] = len(parts)
            parts.append((_turned(r, True), []))
    for i, r in enumerate(rings):
        if depth[i] % 2 == 1:
            shell = [j for j in holders[i] if depth[j] == depth[i] - 1]
            if len(shell) != 1:
                raise ValueError("a hole without a shell: the rings of a polygon cross or share an edge")
            parts[place[shell[0]]][1].append(_turned(r, False))
    return parts


def _rings_of(polygons, p):
    xy, ro, po = polygons.coords, polygons.ring_offsets, polygons.polygon_offsets
    return [xy[ro[j]:ro[j + 1]] for j in range(po[p], po[p + 1])]


def _closed(ring):
    return [[float(x), float(y)] for x, y in ring] + [[float(ring[0, 0]), float(ring[0, 1])]]


def to_wkt(polygons):
    """One WKT string per polygon of the set: POLYGON when it has one shell, MULTIPOLYGON when several, POLYGON EMPTY when no
    ring.  PolygonSet.from_wkt of the list gives a set that rasterizes to the same grid."""
    def ring(r):
        return "(" + ", ".join(f"{x!r} {y!r}" for x, y in _closed(r)) + ")"

    def part(shell, holes):
        return "(" + ", ".join(ring(r) for r in [shell] + holes) + ")"

    out = []
    for p in range(polygons.num_polygons):
        parts = _parts(_rings_of(polygons, p)) if polygons.polygon_offsets[p + 1] > polygons.polygon_offsets[p] else []
        if not parts:
            out.append("POLYGON EMPTY")
        elif len(parts) == 1:
            out.append("POLYGON " + part(*parts[0]))
        else:
            out.append("MULTIPOLYGON (" + ", ".join(part(*q) for q in parts) + ")")
    return out


def _json_value(v):
    v = v.item() if hasattr(v, "item") else v
    return None if isinstance(v, float) and v != v else v


def write_geojson_polygons(path, polygons, properties=None):
    """Writes the set as a GeoJSON FeatureCollection, one Feature per polygon: a Polygon when it has one shell, else a
    MultiPolygon.  properties: a dict of per-polygon columns (sequences of num_polygons entries), for example the arrays of
    Pipeline.zonal(i) selected by `values - 1` for the crowns of a tree-id band; "value" is the set's own values (p + 1 when it has
    none) unless the dict brings its own.  NaN is written as null.  read_geojson_polygons(path, "value") gives back a set that
    rasterizes to the same grid."""
    P = polygons.num_polygons
    columns = {"value": polygons.values if polygons.values is not None else np.arange(1, P + 1, dtype=np.float32)}
    for name, column in (properties or {}).items():
        if len(column) != P:
            raise ValueError(f"write_geojson_polygons: property {name!r} has {len(column)} entries for {P} polygons")
        columns[name] = column
    features = []
    for p in range(P):
        parts = [[_closed(shell)] + [_closed(h) for h in holes] for shell, holes in _parts(_rings_of(polygons, p))] \
            if polygons.polygon_offsets[p + 1] > polygons.polygon_offsets[p] else []
        if len(parts) == 1:
            geometry = {"type": "Polygon", "coordinates": parts[0]}
        else:
            geometry = {"type": "MultiPolygon", "coordinates": parts}
        features.append({"type": "Feature", "properties": {k: _json_value(c[p]) for k, c in columns.items()}, "geometry": geometry})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)


PolygonSet.from_wkt = staticmethod(from_wkt)
PolygonSet.to_wkt = to_wkt
