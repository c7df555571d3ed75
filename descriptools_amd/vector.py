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
    zonal.statistics(zones, hand, len(g["properties"]))                   # row k belongs to properties[k]

POLYGONISATION (what gdal_polygonize and rasterio.features.shapes do): the way back off the grid, and the inverse of the
polygon fill above -- rasterize(polygonize(labels).geometry, labels.shape) equals where(labels >= 0, labels, -1) bit for
bit.  THIS definition is the contract and tests/_polygonize_ref.py is its reference: the library matches it byte for byte.

polygonize(labels, background=None, return_info=False) -> Polygons(geometry, shell).
Input.  labels is a 2-D bool or integer raster, H x W, of fewer than 2^31 cells.  A negative value is background;
background=v makes the value v background too (a mask is polygonize(mask, background=0)); everything else must lie in
[0, 2^30] (MAX_ID), else ValueError before any library call.  Float rasters are refused as in `regions`: compare first.
The library is handed int32 with -1 on background.  Outside the raster is background.
Boundary edges.  A unit edge of the cell lattice, raster border included, between two cells whose labels differ carries
one directed edge for each side that is not background, directed so that its own cell lies on the right of the direction
of travel as seen with x to the right and y down: a cell's top edge travels east, its right edge south, its bottom edge
west, its left edge north.  An edge between two cells of one label carries nothing.
Successor.  At its head vertex a directed edge of label L goes on into the directed edge of L that leaves that vertex;
where two leave -- L's cells meet only diagonally there -- the ring turns right.  So a ring stays with its own cell and
never crosses itself or another ring of L; every 4-connected region of a label has exactly one outer ring (a shell) and
one ring per hole; regions that touch only diagonally are separate shells of one id that share a vertex, which under
rasterize's even-odd rule is the same cell set.
Rings.  Each cycle of the successor relation is one part.  Only the vertices where the direction changes are kept, so
every ring has an even number of at least 4 vertices, alternately joined by horizontal and vertical runs.  The ring
starts at its lexicographically smallest (y, x) vertex, which is always a corner, and follows the direction of travel:
a shell leaves its start eastward and has positive shoelace area in (x, y), a hole leaves it southward and has negative
area.  With a north-up geotransform the shells are counter-clockwise in world coordinates, as RFC 7946 asks.
Coordinates are the integers of the lattice as float64 pixel-corner coordinates: geometry is Geometry("polygon", coords,
parts, ids) with ids[p] the label of ring p.
Order of parts.  Ascending start vertex y * (W + 1) + x, and at one vertex the shell before the hole (at most one of
each can start at a vertex: the ring leaves it along the one east edge or the one south edge that start there).
shell.  int32[P]: the position of the part that is the outer ring of the ring's 4-connected region, the part itself for a
shell.  For a hole h of label L the cell directly above its start vertex (row y - 1, column x) has label L; walk west
from it along its row to the first cell that is not L, or to the border; the vertical edge crossed belongs to a ring of
the same region: a shell, which is h's, or a hole with a strictly smaller start vertex, whose shell h inherits.
info (return_info=True): {"edges", "vertices", "rings", "holes", "rounds"}: directed edges, kept vertices, parts, the
parts that are holes, and the rounds of pointer doubling that found the rings' start vertices, the first round that
lowers no window's smallest start vertex included (round k joins two windows of 2^(k-1) edges).
An all-background raster gives the empty geometry: P = 0, parts == [0].

from_pixel inverts to_pixel; to_geojson writes Polygons (shells followed by their holes), lines and points as a GeoJSON
FeatureCollection, one Feature per id.  Recipes:
    extent = regions.connected(hand <= h, river == 1)                     # a flood extent layer
    vector.to_geojson(vector.polygonize(extent, background=0), geotransform, path="extent.geojson")
    zones, table = zonal.compact(watershed.basins(fdr))                   # basins: properties from the table
    vector.to_geojson(vector.polygonize(zones), geotransform, {k: {"basin": int(v)} for k, v in enumerate(table)})
    zones, table = zonal.compact(regions.label(mask))                     # one feature per connected region
    vector.polygonize(zones)"""
import json
import math
from collections import namedtuple

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


# ---- polygonisation -----------------------------------------------------------------------------------------------------
Polygons = namedtuple("Polygons", ["geometry", "shell"])

_INFO = ("edges", "vertices", "rings", "holes", "rounds")


def _labels(labels, background):
    """labels as int32 with -1 on background; ValueError for what the module docstring refuses"""
    a = _args.raster(labels, "labels", kinds="biu")
    valid = np.ones(a.shape, bool) if a.dtype.kind in "bu" else a >= 0
    if background is not None:
        if not isinstance(background, (int, np.integer)) or isinstance(background, (bool, np.bool_)):
            raise ValueError("background must be an integer or None, not %r" % (background,))
        valid &= a != background
    if valid.any() and int(a[valid].max()) > MAX_ID:
        raise ValueError("labels must lie in [0, 2^30] (or be negative, or equal `background`)")
    out = np.full(a.shape, -1, np.int32)
    out[valid] = a[valid]
    return out


def polygonize(labels, background=None, return_info=False):
    """The rings of a label raster -> Polygons(geometry, shell): geometry a polygon Geometry whose ids are the labels,
    shell int32[P] the position of each ring's outer ring.  The module docstring holds the definition.
    return_info=True -> (polygons, {"edges", "vertices", "rings", "holes", "rounds"})."""
    lab = _labels(labels, background)
    H, W = lab.shape
    L = _lib.lib()
    count = np.zeros(2, np.int64)
    check(L.dt_polygonize_count(ptr(lab, c_i32p), H, W, ptr(count, c_i64p)))
    edges, vertices = int(count[0]), int(count[1])
    if edges >= 2 ** 31:
        raise ValueError("labels has %d directed boundary edges; polygonize takes fewer than 2^31" % edges)
    rings = vertices // 4  # a ring has at least 4 vertices
    coords = host_empty((vertices, 2), np.float64)
    parts, ids, shell = np.zeros(rings + 1, np.int64), np.empty(rings, np.int32), np.empty(rings, np.int32)
    info = np.zeros(8, np.int64)
    check(L.dt_polygonize(ptr(lab, c_i32p), H, W, vertices, rings, ptr(coords, c_f64p), ptr(parts, c_i64p),
                          ptr(ids, c_i32p), ptr(shell, c_i32p), ptr(info, c_i64p)))
    if info[5] != 0 or info[1] != vertices:
        raise RuntimeError("polygonize: the count phase and the call disagree (info = %s)" % info.tolist())
    P = int(info[2])
    out = Polygons(Geometry("polygon", coords, parts[:P + 1].copy(), ids[:P].copy()), shell[:P].copy())
    if return_info:
        return out, dict(zip(_INFO, (int(v) for v in info[:5])))
    return out


def from_pixel(xy, transform):
    """Pixel-corner coordinates xy (float64[..., 2], (x, y)) -> world coordinates (X, Y) of the grid with the GDAL-order
    geotransform (x0, dx, rx, y0, ry, dy), in numpy float64, one rounding per operation, in this association:
        X = (x0 + dx * x) + rx * y        Y = (y0 + ry * x) + dy * y
    -- the inverse of to_pixel, exact when the products and sums are (a north-up transform with power-of-two pixels).
    ValueError as to_pixel."""
    try:
        t = tuple(transform)
    except TypeError:
        t = None
    to_pixel(np.zeros((1, 2)), t)  # the checks, singularity included
    x0, dx, rx, y0, ry, dy = (np.float64(e) for e in t)
    a = np.asarray(xy, np.float64)
    if a.ndim < 1 or a.shape[-1] != 2:
        raise ValueError("xy must have shape (..., 2), not %s" % (a.shape,))
    x, y = a[..., 0], a[..., 1]
    return np.stack(((x0 + dx * x) + rx * y, (y0 + ry * x) + dy * y), axis=-1)


_GEOJSON_TYPE = {"polygon": ("Polygon", "MultiPolygon"), "line": ("LineString", "MultiLineString"),
                 "point": ("Point", "MultiPoint")}


def to_geojson(polygons_or_geometry, transform=None, properties=None, path=None):
    """A GeoJSON FeatureCollection (a dict; written to `path` with `json` when one is given) of a Polygons, or of a line
    or point Geometry: one Feature per distinct id, in ascending id, with properties[id] where `properties` (a mapping or
    a sequence) holds it, else {"id": id}.  Polygons become Polygon or MultiPolygon: each shell in part order followed by
    its holes in part order, grouped through `shell`, every ring closed by repeating its first vertex; lines become
    LineString or MultiLineString, points Point or MultiPoint.  With `transform` (a GDAL geotransform) the coordinates go
    through from_pixel; without, they stay pixel-corner coordinates.  A polygon Geometry comes without the grouping of
    its rings and is refused: polygonize returns it as Polygons(geometry, shell)."""
    if isinstance(polygons_or_geometry, Polygons):
        g, shell = _geometry(polygons_or_geometry.geometry), np.asarray(polygons_or_geometry.shell)
        if g.kind != "polygon":
            raise ValueError("Polygons.geometry must be a polygon geometry, not %r" % g.kind)
        if shell.shape != g.ids.shape or (shell.size and shell.dtype.kind not in "iu"):
            raise ValueError("shell must hold one integer per part (%d), not shape %s" % (g.ids.size, shell.shape))
        if shell.size and (shell.min() < 0 or shell.max() >= shell.size or (shell[shell] != shell).any()
                           or (g.ids[shell] != g.ids).any()):
            raise ValueError("shell must name, for every part, a part of the same id that is its own shell")
    else:
        g, shell = _geometry(polygons_or_geometry), None
        if g.kind == "polygon":
            raise ValueError("a polygon Geometry does not say which rings are holes of which: pass the Polygons(geometry, "
                             "shell) that vector.polygonize returns")
    xy = g.coords if transform is None else from_pixel(g.coords, transform)
    runs = [xy[g.parts[p]:g.parts[p + 1]].tolist() for p in range(g.ids.size)]
    by_id = {}
    if g.kind == "polygon":
        polygon_at = {}
        for p in range(g.ids.size):      # shells in part order, then every hole behind its shell
            if shell[p] == p:
                polygon_at[p] = len(by_id.setdefault(int(g.ids[p]), []))
                by_id[int(g.ids[p])].append([runs[p] + runs[p][:1]])
        for p in range(g.ids.size):
            if shell[p] != p:
                by_id[int(g.ids[p])][polygon_at[int(shell[p])]].append(runs[p] + runs[p][:1])
    else:
        for p in range(g.ids.size):
            members = by_id.setdefault(int(g.ids[p]), [])
            if g.kind == "line":
                members.append(runs[p])
            else:
                members.extend(runs[p])
    features = []
    for k in sorted(by_id):
        members = by_id[k]
        if not members:      # an id whose parts hold no point
            continue
        single, multi = _GEOJSON_TYPE[g.kind]
        geom = {"type": single, "coordinates": members[0]} if len(members) == 1 else {"type": multi, "coordinates": members}
        try:
            props = properties[k]
        except (TypeError, KeyError, IndexError):
            props = {"id": k}
        features.append({"type": "Feature", "properties": props, "geometry": geom})
    out = {"type": "FeatureCollection", "features": features}
    if path is not None:
        with open(path, "w") as f:
            json.dump(out, f)
    return out
