"""Vector rasterisation (net-new; what gdal_rasterize and rasterio.features.rasterize do): polygons, lines and points
burnt onto the grid as an int32 label raster.  Every other op of the package takes rasters; this is the way in for data
that arrives as geometry: benchmark flood extents, river centrelines, levees, gauges, administrative zones.  THIS
definition is the contract and tests/_vector_ref.py is its reference: the library matches it bit for bit.

Geometry(kind, coords, parts, ids) holds one kind of geometry, "polygon", "line" or "point".  coords is float64[N, 2],
column first (x, y), in the pixel-corner coordinates of `resample`: cell (row i, col j) covers [j, j+1) x [i, i+1), its
centre is (j + 0.5, i + 0.5).  parts is int64[P + 1], the offsets of the parts -- a ring, a linestring, a run of points
-- and ids is int32[P], the id each part burns, 0 <= id <= 2^30.  Several rings with one id form one polygon with holes
or a multipolygon: the rule is even-odd over all of them, so holes need no flag and no winding order.  A ring is closed
implicitly: its last vertex is joined to its first.

rasterize -> int32[H, W]: a cell holds the LARGEST id of the parts that burn it, -1 where none does, so the result
depends on no order of work; with ids = position (from_geojson) that is GDAL's "later feature wins".  Cells outside the
raster are dropped.  All arithmetic is float64, one rounding per operation, in the association written here, and every
range is clipped to the raster as float64 BEFORE anything becomes an integer: coordinates of +-10^12 are harmless and
cost nothing.

Polygon interior.  A cell is inside when its centre is inside by the even-odd rule over all rings of the id.  Each edge
is first oriented upward, (xa, ya) the endpoint with the smaller y; an edge with ya == yb crosses nothing.  It crosses the
centre lines of rows r0 <= r < r1, r0 = ceil(ya - 0.5), r1 = ceil(yb - 0.5), clipped to [0, H).  On row r, yc = r + 0.5:
    t = (yc - ya) / (yb - ya)        x = xa + t * (xb - xa)        c = ceil(x - 0.5), clamped to [0, W]
Per (row, id) the crossing columns are sorted and pairs (2k, 2k+1) fill the cells [c_lo, c_hi).  A closed ring under
these half-open rules yields an even count per (row, id).  Edges are oriented before the arithmetic, so an edge shared by
two polygons gives both the same crossing: a tessellation labels every covered cell exactly once.

Lines.  A segment with dx = xb - xa, dy = yb - ya is x-major when |dx| >= |dy| and is then oriented so that xa < xb;
y-major is the same with the roles swapped.  dx == dy == 0 (and a part of one vertex) burns the one cell (floor(ya),
floor(xa)).  For every column c from floor(xa) to floor(xb), clipped to [0, W), with
    y(x) = ya + ((x - xa) / (xb - xa)) * (yb - ya),   y(xa) = ya and y(xb) = yb by rule, not by arithmetic:
  connectivity 4 ("touched")  x_in = max(xa, c), x_out = min(xb, c + 1): rows floor(min(y(x_in), y(x_out))) to
      floor(max(...)) inclusive.  Neighbouring columns evaluate the same expression at their common edge, so the cells
      are 4-connected: a levee drawn this way holds water in inundation.simulate, and no diagonal step (D8, cost
      distance at connectivity 8) slips through it, as one does through a thin line.
  connectivity 8 ("thin")     the one row floor(y(xs)), xs = min(max(c + 0.5, xa), xb), and the two endpoint cells:
      8-connected, what a D8 `river` raster wants.
Points.  A point burns the cell (floor(y), floor(x)).

all_touched=True is the polygon's interior plus its rings burnt as connectivity-4 lines -- "touched" is what
connectivity 4 computes -- whatever `connectivity` says; `connectivity` is the setting of line geometries.

Refused with ValueError before any library call: non-finite coordinates; parts that are not non-decreasing from 0 to N;
an id outside [0, 2^30]; a ring of fewer than 3 vertices, a line part of fewer than 1; a bad shape (resample's rules);
a connectivity other than 4 or 8.  An empty geometry (P = 0) is valid and gives all -1.

Recipes (g = vector.from_geojson(path, rasterio_lite.geotransform(meta))):
    observed = vector.mask(g["polygon"], dem.shape)                       # a benchmark flood extent
    evaluation.calibration(hand, observed, True)
    river = vector.mask(g["line"], dem.shape)                             # hydrography at connectivity 8
    flowhand.flow_hand_index(dem, fdr, river, px)
    burnt = dem - depth * (vector.rasterize(g["line"], dem.shape) >= 0)   # stream burning before d8_conditioned
    wall = vector.mask(levees, dem.shape, connectivity=4)                 # 4-connected: holds water
    inundation.simulate(np.where(wall, -100, dem), px, ...)               # a nodata wall
    cost.cost_distance(np.where(wall, -100, friction), sources, px)       # a barrier
    pour_points = vector.rasterize(g["point"], dem.shape) + 1             # gauges: watersheds wants labels > 0
    zones = vector.rasterize(g["polygon"], dem.shape)                     # admin polygons:
    zonal.statistics(zones, hand, len(g["properties"]))                   # row k belongs to properties[k]"""
import json
import math

import numpy as np

from . import _args, _lib, resample, zonal
from ._lib import c_f64p, c_i32p, c_i64p, check, ptr
from .device import host_empty

KINDS = ("polygon", "line", "point")
MAX_ID = 2 ** 30


class Geometry:
    """One kind of geometry: kind in KINDS, coords float64[N, 2] (x, y) in pixel-corner coordinates, parts int64[P + 1],
    ids int32[P].  ValueError for what the module docstring refuses."""

    __slots__ = ("kind", "coords", "parts", "ids")

    def __init__(self, kind, coords, parts, ids):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, not %r" % (KINDS, kind))
        try:
            c = np.ascontiguousarray(coords, np.float64)
        except (TypeError, ValueError):
            raise ValueError("coords must be an array of numbers of shape (N, 2)") from None
        if c.size == 0:
            c = c.reshape(0, 2)
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError("coords must have shape (N, 2), not %s" % (c.shape,))
        if c.shape[0] >= 2 ** 31:
            raise ValueError("coords holds %d vertices; a geometry must have fewer than 2^31" % c.shape[0])
        if not np.isfinite(c).all():
            raise ValueError("coords must be finite")
        p, i = np.asarray(parts), np.asarray(ids)
        if p.ndim != 1 or p.size < 1 or p.dtype.kind not in "iu":
            raise ValueError("parts must be a 1-D integer array of P + 1 offsets")
        if i.ndim != 1 or i.size != p.size - 1 or (i.size and i.dtype.kind not in "iu"):
            raise ValueError("ids must be a 1-D integer array with one id per part (%d), not of shape %s"
                             % (p.size - 1, i.shape))
        p = np.ascontiguousarray(p, np.int64)
        if p[0] != 0 or p[-1] != c.shape[0] or (np.diff(p) < 0).any():
            raise ValueError("parts must be non-decreasing from 0 to N = %d" % c.shape[0])
        if i.size and (int(i.min()) < 0 or int(i.max()) > MAX_ID):
            raise ValueError("ids must lie in [0, 2^30]")
        n = np.diff(p)
        if kind == "polygon" and (n < 3).any():
            raise ValueError("a ring must have at least 3 vertices")
        if kind == "line" and (n < 1).any():
            raise ValueError("a line part must have at least 1 vertex")
        self.kind, self.coords, self.parts, self.ids = kind, c, p, np.ascontiguousarray(i, np.int32)

    def __repr__(self):
        return "Geometry(%r, %d vertices, %d parts)" % (self.kind, self.coords.shape[0], self.ids.size)


def _geometry(g):
    """g checked again: its arrays may have changed since it was made"""
    if not isinstance(g, Geometry):
        raise ValueError("geometry must be a vector.Geometry, not %r" % type(g).__name__)
    return Geometry(g.kind, g.coords, g.parts, g.ids)


def to_pixel(xy, transform):
    """World coordinates xy (float64[..., 2], (X, Y)) -> pixel-corner coordinates (x, y) of the grid with the
    GDAL-order geotransform (x0, dx, rx, y0, ry, dy), in numpy float64 with det = dx*dy - rx*ry:
        x = (dy*(X - x0) - rx*(Y - y0)) / det        y = (dx*(Y - y0) - ry*(X - x0)) / det
    -- the association of resample.compose.  ValueError for a transform that is not six finite numbers or is singular."""
    try:
        t = tuple(math.nan if isinstance(e, (bool, np.bool_)) else float(e) for e in transform)
    except (TypeError, ValueError):
        t = ()
    if len(t) != 6 or not all(math.isfinite(e) for e in t):
        raise ValueError("transform must be six finite numbers (x0, dx, rx, y0, ry, dy), not %r" % (transform,))
    x0, dx, rx, y0, ry, dy = (np.float64(e) for e in t)
    det = dx * dy - rx * ry
    if not (np.isfinite(det) and det != 0.0):
        raise ValueError("transform %r is singular" % (t,))
    a = np.asarray(xy, np.float64)
    if a.ndim < 1 or a.shape[-1] != 2:
        raise ValueError("xy must have shape (..., 2), not %s" % (a.shape,))
    ex, ey = a[..., 0] - x0, a[..., 1] - y0
    return np.stack(((dy * ex - rx * ey) / det, (dx * ey - ry * ex) / det), axis=-1)


_GEOJSON_KIND = {"Point": "point", "MultiPoint": "point", "LineString": "line", "MultiLineString": "line",
                 "Polygon": "polygon", "MultiPolygon": "polygon"}


def _geojson_parts(g):
    """[(kind, [vertex list, ...])] of a GeoJSON geometry object"""
    t, c = g.get("type"), g.get("coordinates")
    if t == "GeometryCollection":
        return [e for sub in g.get("geometries", ()) for e in _geojson_parts(sub)]
    if t not in _GEOJSON_KIND:
        raise ValueError("GeoJSON geometry type %r is not supported" % (t,))
    if t == "Point":
        runs = [[c]]
    elif t in ("MultiPoint", "LineString"):
        runs = [c]
    elif t in ("MultiLineString", "Polygon"):
        runs = list(c)
    else:
        runs = [ring for poly in c for ring in poly]
    if t in ("Polygon", "MultiPolygon"):  # GeoJSON repeats a ring's first vertex at its end; the closing is implicit here
        runs = [r[:-1] if len(r) > 3 and list(r[0][:2]) == list(r[-1][:2]) else r for r in runs]
    return [(_GEOJSON_KIND[t], runs)]


def from_geojson(obj_or_path, transform=None):
    """A GeoJSON object (a dict) or file (a path), read with `json` alone: Point, MultiPoint, LineString,
    MultiLineString, Polygon, MultiPolygon, Feature, FeatureCollection -> {"polygon": Geometry or None, "line": ...,
    "point": ..., "properties": [...]}.  A part's id is its feature's position in the collection, so properties[label]
    is the attribute lookup.  With `transform` (a GDAL geotransform) the coordinates go through to_pixel; without, they
    are taken as pixel-corner coordinates."""
    if isinstance(obj_or_path, dict):
        obj = obj_or_path
    else:
        with open(obj_or_path) as f:
            obj = json.load(f)
    t = obj.get("type")
    if t == "FeatureCollection":
        features = list(obj.get("features", ()))
    elif t == "Feature":
        features = [obj]
    else:
        features = [{"type": "Feature", "geometry": obj, "properties": None}]
    acc = {k: ([], [0], []) for k in KINDS}
    for pos, f in enumerate(features):
        if f.get("geometry") is None:
            continue
        for kind, runs in _geojson_parts(f["geometry"]):
            xy, parts, ids = acc[kind]
            for r in runs:
                try:
                    xy.extend((float(v[0]), float(v[1])) for v in r)
                except (TypeError, ValueError, IndexError):
                    raise ValueError("feature %d holds a position that is not two numbers" % pos) from None
                parts.append(len(xy))
                ids.append(pos)
    out = {"properties": [f.get("properties") for f in features]}
    for kind, (xy, parts, ids) in acc.items():
        if not ids:
            out[kind] = None
            continue
        c = np.array(xy, np.float64).reshape(-1, 2)
        out[kind] = Geometry(kind, c if transform is None else to_pixel(c, transform), parts, ids)
    return out


def _call(geometry, shape, connectivity, all_touched):
    g = _geometry(geometry)
    H, W = resample._shape(shape)
    conn = _args.connectivity(connectivity)
    if not isinstance(all_touched, (bool, np.bool_)):
        raise ValueError("all_touched must be a bool, not %r" % (all_touched,))
    return g, H, W, conn, int(all_touched)


def count_crossings(geometry, shape):
    """(total, largest_row): the crossings of a polygon geometry's edges with the centre lines of the raster's rows --
    the exact work and scratch count of rasterize, 8 bytes each -- and the most on any one row; (0, 0) for lines and
    points.  Host arithmetic: no device is needed."""
    g, H, W, _, _ = _call(geometry, shape, 8, False)
    total, largest = np.zeros(1, np.int64), np.zeros(1, np.int64)
    check(_lib.lib().dt_rasterize_count(KINDS.index(g.kind), ptr(g.coords, c_f64p), ptr(g.parts, c_i64p), g.ids.size, H,
                                        W, ptr(total, c_i64p), ptr(largest, c_i64p)))
    return int(total[0]), int(largest[0])


def rasterize(geometry, shape, connectivity=8, all_touched=False, return_info=False):
    """The label raster of `geometry` on a grid of `shape` = (H, W) -> int32[H, W]: the largest id that burns a cell, -1
    where none does.  The module docstring holds the definition.  return_info=True -> (label, {"crossings",
    "largest_row", "slow_rows", "overflow"}): slow_rows counts the rows whose crossings did not fit LDS and were sorted
    in global memory."""
    g, H, W, conn, touched = _call(geometry, shape, connectivity, all_touched)
    label = host_empty((H, W), np.int32)
    info = np.zeros(4, np.int64)
    check(_lib.lib().dt_rasterize(KINDS.index(g.kind), ptr(g.coords, c_f64p), ptr(g.parts, c_i64p), ptr(g.ids, c_i32p),
                                  g.ids.size, H, W, conn, touched, ptr(label, c_i32p), ptr(info, c_i64p)))
    if return_info:
        return label, dict(zip(("crossings", "largest_row", "slow_rows", "overflow"), (int(v) for v in info)))
    return label


def mask(geometry, shape, connectivity=8, all_touched=False):
    """uint8[H, W]: 1 where rasterize(...) >= 0"""
    return (rasterize(geometry, shape, connectivity, all_touched) >= 0).astype(np.uint8)


def burn(geometry, shape, values, fill, connectivity=8, all_touched=False):
    """values[id] burnt where rasterize(...) holds id, `fill` elsewhere and where id >= len(values):
    zonal.paint(values, label, fill), in the dtype of `values`"""
    return zonal.paint(values, rasterize(geometry, shape, connectivity, all_touched), fill)
