"""Raster resampling (net-new; what GDAL's warp and ArcGIS's Resample / Aggregate do): a raster on one grid read onto
another.  Every other op of the package assumes that its rasters share one grid; this is the op that puts them there:
a benchmark flood map on the DEM's grid, a DEM coarsened for a cheaper simulation and the water surface brought back,
the same descriptor at 10, 30 and 90 m.  THIS definition is the contract and tests/_resample_ref.py is its reference:
the library matches it bit for bit.

Coordinates are pixel-corner coordinates, column first: cell (row i, col j) covers [j, j+1) x [i, i+1), its centre is
(j + 0.5, i + 0.5).  `matrix` = (a0, a1, a2, b0, b1, b2) maps destination pixel coordinates (x, y) to source pixel
coordinates
    u = (a0 + a1*x) + a2*y        v = (b0 + b1*x) + b2*y
All arithmetic is float64 with one rounding per operation in the association written here (the library is built without
contraction).  A float32 raster is taken to float64, which is exact, and the result is rounded to float32 once.  A
float cell is VALID iff it is finite and > -100; float outputs hold -100 where they have no value.

Point methods take any non-singular matrix (rotation, flips).  (u, v) is evaluated at the destination centre x = j +
0.5, y = i + 0.5; with c = floor(u), r = floor(v) the cell is OUTSIDE unless 0 <= u < Ws and 0 <= v < Hs, compared as
float64 before anything becomes an integer.
  nearest   copies the bits of src[r, c]: any dtype of item size 1, 2, 4 or 8 (bool, every integer, the int64 labels of
            watershed.basins, float32, float64), no validity test.  Outside cells take `fill`: by default -100 for
            signed and float dtypes, 0 for unsigned and bool.
  bilinear  float32 / float64.  No value outside, and none when the containing cell src[r, c] is invalid: values never
            bleed into nodata.  Otherwise u' = u - 0.5, c0 = floor(u'), fx = u' - c0, likewise v', r0, fy; the taps are
            (r0, c0), (r0, c0+1), (r0+1, c0), (r0+1, c0+1) in that order with w = wy*wx, wx in (1 - fx, fx), wy in
            (1 - fy, fy).  A tap counts iff w != 0, it lies in the raster and it is valid.  S = sum of w*z and D = sum of
            w over the counting taps, each summed in order from 0; the value is S/D.  The containing cell always counts
            with w >= 0.25, so D > 0.
  cubic     Keys' kernel with a = -0.5, in Horner form: the weights of columns c0-1 .. c0+2 are
                kf(1 + fx), kn(fx), kn(1 - fx), kf(2 - fx)
                kn(t) = ((1.5*t - 2.5)*t)*t + 1          kf(t) = ((-0.5*t + 2.5)*t - 4)*t + 2
            and likewise for rows r0-1 .. r0+2 with fy.  When all 16 taps are in the raster and valid the value is the sum
            over the rows, top to bottom from 0, of wy * (the sum over the columns, left to right from 0, of wx*z); no
            renormalisation.  Otherwise the cell takes the bilinear value.

Area methods take an axis-aligned matrix: a2 == b1 == 0, a1 > 0, b2 > 0, and a1 <= 256, b2 <= 256 (chain two calls for
more).  Destination cell (i, j) covers [u0, u1) x [v0, v1) with u0 = a0 + a1*j, u1 = a0 + a1*(j+1) -- one expression for
a cell's right edge and its neighbour's left edge -- and v0 = b0 + b2*i, v1 = b0 + b2*(i+1).  Source column c has the
weight wx = min(u1, c+1) - max(u0, c) and is TAKEN iff 0 <= c < Ws and wx > 0; rows likewise with wy.
  average, sum   float32 / float64.  Rows top to bottom; in a row s = d = 0, then s = s + wx*z and d = d + wx for every
            valid taken cell, left to right; then S = S + wy*s and D = D + wy*d.  A value iff D > 0: S/D, or S.
  min, max  float32 / float64: the extreme of the valid taken cells, in row-major order, the first of equal values
            (-0.0 == 0.0); no value without such a cell.
  mode      uint8 only: the most frequent value among the taken cells, the smallest on a tie.  Cells equal to the
            optional integer `nodata` are not counted; a destination cell without a counted cell takes `fill` (0 by
            default).

Refused with ValueError before any library call: a raster that is not 2-D, 2^31 cells or more on either side, an empty
shape; a matrix that is not six finite numbers or is singular; a method / dtype pair outside the lists above; a rotated
or flipped matrix with an area method, or its cap of 256 exceeded; a `fill` or `nodata` outside the dtype, a `fill` with a
method that writes -100, a `nodata` with a method other than mode.

Recipes.  A benchmark flood map on the DEM's grid ("nearest" for labels, "bilinear" for depths):
    flood = resample.align(flood_map, rasterio_lite.geotransform(m_flood), rasterio_lite.geotransform(m_dem),
                           dem.shape, "mode")
Coarse simulation, fine map:
    dem_c = resample.aggregate(dem, 4, "average")
    res = inundation.simulate(dem_c, 4 * px, ...)
    wse_c = np.where(res.max_depth > 0, dem_c + res.max_depth, -100)
    wse = resample.resize(wse_c, dem.shape, "bilinear")
    depth = np.where(wse > -100, np.maximum(wse - dem, 0), 0)
The flooded fraction of a coarse cell: aggregate(hand <= h, k, "average") on a float raster; class rasters coarsen with
aggregate(landform, k, "mode")."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f64p, check
from .device import host_empty

METHODS = ("nearest", "bilinear", "cubic", "average", "sum", "min", "max", "mode")
AREA_METHODS = METHODS[3:]
MAX_FOOTPRINT = 256


def _matrix(matrix):
    try:
        m = tuple(math.nan if isinstance(v, (bool, np.bool_)) else float(v) for v in matrix)
    except (TypeError, ValueError):
        m = ()
    if len(m) != 6 or not all(math.isfinite(v) for v in m):
        raise ValueError("matrix must be six finite numbers (a0, a1, a2, b0, b1, b2), not %r" % (matrix,))
    det = m[1] * m[5] - m[2] * m[4]
    if not (math.isfinite(det) and det != 0.0):
        raise ValueError("matrix %r is singular" % (m,))
    return m


def _shape(shape, what="shape"):
    try:
        h, w = shape
    except (TypeError, ValueError):
        raise ValueError("%s must be (rows, cols), not %r" % (what, shape))
    h, w = _args.integer(h, what + "[0]", 1, 2 ** 31 - 1), _args.integer(w, what + "[1]", 1, 2 ** 31 - 1)
    if h * w >= _args.MAX_CELLS:
        raise ValueError("%s %r has %d cells; a raster must have fewer than 2^31" % (what, (h, w), h * w))
    return h, w


def _element(v, dtype, what):
    """v as one element of dtype, ValueError when the dtype cannot hold it"""
    if dtype.kind == "f":
        try:
            f = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, not %r" % (what, v))
        with np.errstate(over="ignore"):
            e = np.array(f, dtype)
        if math.isfinite(f) and float(e) != f:
            raise ValueError("%s=%r is not a %s value" % (what, v, dtype))
        return e
    if dtype.kind == "b":
        if not (isinstance(v, (bool, np.bool_)) or (_args._is_int(v) and int(v) in (0, 1))):
            raise ValueError("%s=%r is not a bool value" % (what, v))
        return np.array(bool(v), dtype)
    info = np.iinfo(dtype)
    if not _args._is_int(v) or not info.min <= int(v) <= info.max:
        raise ValueError("%s=%r is not a %s value" % (what, v, dtype))
    return np.array(int(v), dtype)


def _code(method, dtype):
    """the library's dtype code of a method / dtype pair, ValueError outside the lists of the module docstring"""
    if method == "nearest":
        if dtype.kind in "biuf" and dtype.itemsize in (1, 2, 4, 8):
            return dtype.itemsize
    elif method == "mode":
        if dtype == np.uint8:
            return 1
    elif dtype in (np.float32, np.float64):
        return 32 if dtype == np.float32 else 64
    raise ValueError("method %r does not take dtype %s" % (method, dtype))


def warp(src, matrix, shape, method="nearest", nodata=None, fill=None):
    """`src` read onto a destination grid of `shape` = (H, W) through `matrix` = (a0, a1, a2, b0, b1, b2), which maps
    destination to source pixel coordinates -> an array of src's dtype.  The module docstring holds the definition of
    every method."""
    if method not in METHODS:
        raise ValueError("method must be one of %s, not %r" % (METHODS, method))
    a = _args.raster(src, "src")
    if a.size == 0:
        raise ValueError("src is empty: shape %s" % (a.shape,))
    m = _matrix(matrix)
    Hd, Wd = _shape(shape)
    dt = a.dtype
    code = _code(method, dt)
    if method in AREA_METHODS:
        if not (m[2] == 0.0 and m[4] == 0.0 and m[1] > 0.0 and m[5] > 0.0):
            raise ValueError("method %r takes an axis-aligned matrix (a2 == b1 == 0, a1 > 0, b2 > 0), not %r"
                             % (method, m))
        if m[1] > MAX_FOOTPRINT or m[5] > MAX_FOOTPRINT:
            raise ValueError("method %r takes at most %d source cells per destination cell and axis, the matrix asks "
                             "for %g x %g: chain two calls" % (method, MAX_FOOTPRINT, m[5], m[1]))
    if nodata is not None and method != "mode":
        raise ValueError("nodata is mode's; method %r tells nodata by the value (finite and > -100)" % method)
    nd = -1 if nodata is None else int(_element(nodata, dt, "nodata"))
    if method in ("nearest", "mode"):
        default = 0 if dt.kind in "bu" else -100
        fe = _element(default if fill is None else fill, dt, "fill")
    elif fill is not None:
        raise ValueError("fill is nearest's and mode's; method %r writes -100 where it has no value" % method)
    else:
        fe = np.array(-100, dt)
    bits = int.from_bytes(fe.tobytes(), "little")
    a = np.ascontiguousarray(a)
    Hs, Ws = a.shape
    out = host_empty((Hd, Wd), dt)
    mat = np.array(m, np.float64)
    check(_lib.lib().dt_resample(a.ctypes.data, code, Hs, Ws, _lib.ptr(mat, c_f64p), METHODS.index(method), nd, bits,
                                 out.ctypes.data, Hd, Wd))
    return out


def compose(src_transform, dst_transform):
    """The matrix that takes destination pixel coordinates to source pixel coordinates, from two GDAL-order
    geotransforms (x0, dx, rx, y0, ry, dy): X = x0 + dx*col + rx*row, Y = y0 + ry*col + dy*row.  In Python floats,
    with (x0, dx, rx, y0, ry, dy) the source's, (X0, DX, RX, Y0, RY, DY) the destination's and det = dx*dy - rx*ry:
        a0 = (dy*(X0 - x0) - rx*(Y0 - y0)) / det      b0 = (dx*(Y0 - y0) - ry*(X0 - x0)) / det
        a1 = (dy*DX - rx*RY) / det                    b1 = (dx*RY - ry*DX) / det
        a2 = (dy*RX - rx*DY) / det                    b2 = (dx*DY - ry*RX) / det
    ValueError for a transform that is not six finite numbers or is singular (either one)."""
    def six(t, what):
        try:
            v = tuple(math.nan if isinstance(e, (bool, np.bool_)) else float(e) for e in t)
        except (TypeError, ValueError):
            v = ()
        if len(v) != 6 or not all(math.isfinite(e) for e in v):
            raise ValueError("%s must be six finite numbers (x0, dx, rx, y0, ry, dy), not %r" % (what, t))
        d = v[1] * v[5] - v[2] * v[4]
        if not (math.isfinite(d) and d != 0.0):
            raise ValueError("%s %r is singular" % (what, v))
        return v, d
    (x0, dx, rx, y0, ry, dy), det = six(src_transform, "src_transform")
    (X0, DX, RX, Y0, RY, DY), _ = six(dst_transform, "dst_transform")
    ex, ey = X0 - x0, Y0 - y0
    return ((dy * ex - rx * ey) / det, (dy * DX - rx * RY) / det, (dy * RX - rx * DY) / det,
            (dx * ey - ry * ex) / det, (dx * RY - ry * DX) / det, (dx * DY - ry * RX) / det)


def align(src, src_transform, dst_transform, dst_shape, method="nearest", nodata=None, fill=None):
    """`src`, georeferenced by `src_transform`, on the grid of `dst_transform` and `dst_shape`:
    warp(src, compose(src_transform, dst_transform), dst_shape, ...)"""
    return warp(src, compose(src_transform, dst_transform), dst_shape, method, nodata, fill)


def resize(src, shape, method="nearest", nodata=None, fill=None):
    """The extent of `src` on a grid of another `shape`: the matrix is (0, Ws/Wd, 0, 0, 0, Hs/Hd)"""
    a = _args.raster(src, "src")
    Hd, Wd = _shape(shape)
    return warp(a, (0.0, a.shape[1] / Wd, 0.0, 0.0, 0.0, a.shape[0] / Hd), (Hd, Wd), method, nodata, fill)


def aggregate(src, factor, how="average", nodata=None, fill=None):
    """Integer block reduction: blocks of `factor` (one integer, or (fy, fx)) cells reduced by the area method `how`
    -> ceil(Hs/fy) x ceil(Ws/fx); the last block of a row or column is the part of it inside the raster"""
    if how not in AREA_METHODS:
        raise ValueError("how must be one of %s, not %r" % (AREA_METHODS, how))
    a = _args.raster(src, "src")
    fy, fx = factor if isinstance(factor, (tuple, list)) and len(factor) == 2 else (factor, factor)
    fy, fx = _args.integer(fy, "factor", 1), _args.integer(fx, "factor", 1)
    shape = (-(-a.shape[0] // fy), -(-a.shape[1] // fx))
    return warp(a, (0.0, float(fx), 0.0, 0.0, 0.0, float(fy)), shape, how, nodata, fill)
