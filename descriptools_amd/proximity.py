"""Exact Euclidean nearest-river distance, allocation and HAND (net-new; the GIS "Euclidean distance / allocation" and
"elevation above stream, Euclidean"): the straight-line twins of flowhand.flow_hand_index's flow distance, drained-to
river index and HAND.  They need only `river`, so they work where no trustworthy flow direction exists.

Inputs.  `river`: a 2-D raster.  `px`: finite and > 0.  `dem`: optional, of river's shape.

Sources and nodata.  A source is a cell with river == 1 (the rule of the flow-path HAND; the raster is taken as int8,
like flow_hand_index takes it).  When `dem` is given, a cell that _lib.nodata_mask calls nodata (dem <= -100, compared in
the DEM's own dtype; NaN is not nodata) is never a source, and gets -100 in every output.  Nodata is not a barrier:
distances are straight lines over it.

Nearest source.  For a cell c = (y, x) and a source s = (ys, xs), d2(c, s) = (y - ys)^2 + (x - xs)^2, an exact integer.
nearest(c) is the source with the smallest d2; among equals it is the one with the smallest flat index ys * W + xs.

Outputs.  indices (int64): the flat index of nearest(c); -100 when the raster has no source or c is nodata; a source's
index is itself.  distance (float32): float32(px * sqrt(float64(d2))), both operations in float64 with one rounding to
float32 at the end; -100 where indices is -100.  hand: exactly flowhand.hand_calculator(dem, indices) -- the DEM's dtype,
and a DEM that float32 cannot hold takes hand_calculator's float64 route.

Refused with ValueError before any library call: rasters of 2^31 cells or more, a raster that is not 2-D, shapes that
differ between river and dem, a px that is not finite and > 0.  (With H * W < 2^31 every d2 < 2^62 fits int64, and so
does the "no source in this row" sentinel 2^62 plus dy^2.)

The result is unique, so it is held bit for bit against a brute-force reference; it does not depend on order or run.
The work is O(H W log H) whatever the sources are (csrc/dt_proximity.hip: a row pass, then a divide-and-conquer column
pass on the Monge cost matrix).  The library sees nodata in one form, a float32 raster whose cells <= -100 are nodata:
the DEM itself when float32 holds every height (the comparison is then the DEM's own), else _lib.nodata_mask(dem).

euclidean_hand's indices are the documented way to the Euclidean variants of everything built on the index raster:
gfi.gfi_calculator(hand, fac, indices, ...), gfi.river_accumulation(fac, indices), reaches.catchments(link, indices)."""
import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_i8p, c_i64p, check, ptr
from .device import host_empty
from .flowhand import hand_calculator


class Proximity(tuple):
    """(distance float32, indices int64) of nearest_river"""
    __slots__ = ()

    def __new__(cls, distance, indices):
        return tuple.__new__(cls, (distance, indices))

    distance = property(lambda self: self[0])
    indices = property(lambda self: self[1])


def nearest_river(river, px, dem=None):
    """Euclidean distance to, and flat index of, the nearest river cell -> Proximity(distance float32, indices int64);
    the module docstring holds the definition.  `dem` (optional) only says which cells are nodata."""
    r = _args.raster(river, "river")
    p = _args.pixel_size(px)
    if dem is not None and np.shape(dem) != r.shape:
        raise ValueError("dem has shape %s, river %s" % (np.shape(dem), r.shape))
    nod = None
    if dem is not None:
        nod, wide = _lib.heights(dem)
        if wide:  # float32(dem) <= -100 is not dem <= -100
            nod = _lib.nodata_mask(dem, r.shape)
    r = np.ascontiguousarray(r, np.int8)
    H, W = r.shape
    distance = host_empty((H, W), np.float32)
    indices = host_empty((H, W), np.int64)
    check(_lib.lib().dt_proximity(ptr(r, c_i8p), ptr(nod, c_f32p), H, W, p, ptr(distance, c_f32p),
                                  ptr(indices, c_i64p)))
    return Proximity(distance, indices)


def euclidean_hand(dem_raster, river_matrix, px):
    """The Euclidean twin of flowhand.flow_hand_index -> (distance float32, indices int64, hand in the DEM's dtype),
    the same -100 conventions: hand is the height above the nearest river cell in a straight line."""
    distance, indices = nearest_river(river_matrix, px, dem=dem_raster)
    return distance, indices, hand_calculator(dem_raster, indices)
