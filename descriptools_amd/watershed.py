"""Drainage basins, pour-point watersheds, flow length to the outlet and upslope (longest) flow length of a D8 raster
(net-new), on the GPU.

Definition (the kernels in csrc/dt_watershed.hip, the C header and the tests hold to it):

* Drainage graph.  Nodes: every cell; when dem is given, cells with dem <= -100 are nodata (the mask
  flowacc.accumulate builds, in the DEM's own dtype: NaN is not nodata).  A cell c has the edge c -> d when its code is
  one of the eight ESRI D8 codes (1 E, 2 SE, 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE), d lies in the raster and, when dem
  is given, neither c nor d is nodata.  A valid cell with no edge is a terminal (outlet): a code of 0 or any non-D8
  value, a code pointing off the raster, or a code pointing into nodata.  This differs on purpose from accumulate,
  where nodata cells pass their inflow on: here a basin ends at nodata.  Without dem the graph is exactly
  accumulate's D8 tree.
* Path and length.  The path of c is c, succ(c), ...; it is finite if it reaches a terminal, otherwise it enters a D8
  cycle.  A stretch of path with n_card cardinal and n_diag diagonal moves is float64(n_card) * px +
  float64(n_diag) * (px * sqrt(2.0)) long, evaluated in float64 in exactly that association on exact integer move
  counts, so lengths are bit-exact and do not depend on order, tiling or run.

Bad arguments raise ValueError before any library call: fdr that is not 2-D, dem or pour_points of another shape,
pour_points of a non-integer dtype or with negative labels, px that is not finite and > 0, a raster of 2^31 cells or
more.

Users of a resident chain call dt_dev_drainage / dt_dev_upslope_length on chain.p("fdr")."""
from collections import namedtuple

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i64p, c_u8p, check, nodata_mask, ptr

Drainage = namedtuple("Drainage", ["target", "length"])


def _checked(fdr, px, dem=None, pour_points=None):
    """(fdr uint8, px float, dem nodata mask float32 or None, pour labels int64 or None), all C-contiguous;
    ValueError before any library call"""
    f = _args.raster(fdr, "fdr", dtype=np.uint8)
    p = _args.pixel_size(px)
    d = nodata_mask(dem, f.shape)  # the DEM is only a nodata mask here, as accumulate takes it
    pp = None
    if pour_points is not None:
        a = _args.raster(pour_points, "pour_points", f.shape, "the direction raster", kinds="iu")
        if a.size and a.dtype.kind == "i" and int(a.min()) < 0:
            raise ValueError("pour point labels must be >= 0 (the smallest is %d)" % int(a.min()))
        if a.size and int(a.max()) > np.iinfo(np.int64).max:
            raise ValueError("pour point labels must fit int64 (the largest is %d)" % int(a.max()))
        pp = np.ascontiguousarray(a, np.int64)
    return f, p, d, pp


def drainage(fdr, px=1.0, dem=None, pour_points=None):
    """Drainage(target, length) of every cell of the D8 raster fdr (see the module docstring for the graph).

    target (int64): the flat index y * W + x of the cell where c's path stops: with pour_points, the first cell on the
    path (c included) whose label is > 0; without, the path's terminal.  length (float64): the length from c to
    target, 0 when c is its own target.  Both are -100 on nodata, where the path enters a D8 cycle before it stops,
    and (with pour_points) where the path ends at a terminal without meeting a pour point.  Pour points on nodata
    cells are ignored."""
    f, p, d, pp = _checked(fdr, px, dem, pour_points)
    H, W = f.shape
    tg = np.empty((H, W), np.int64)
    ln = np.empty((H, W), np.float64)
    check(_lib.lib().dt_drainage(ptr(f, c_u8p), ptr(d, c_f32p), ptr(pp, c_i64p), H, W, p, ptr(tg, c_i64p),
                                 ptr(ln, c_f64p), None))
    return Drainage(tg, ln)


def basins(fdr, dem=None):
    """Basin label (int64) of every cell: the flat index y * W + x of its outlet (drainage(...).target without pour
    points, the convention streams uses for link heads); -100 on nodata and where the path enters a D8 cycle."""
    f, p, d, _ = _checked(fdr, 1.0, dem)
    H, W = f.shape
    tg = np.empty((H, W), np.int64)
    check(_lib.lib().dt_drainage(ptr(f, c_u8p), ptr(d, c_f32p), None, H, W, p, ptr(tg, c_i64p), None, None))
    return tg


def watersheds(fdr, pour_points, dem=None):
    """Watershed label (int64) of every cell: the label of the first pour point (label > 0) on its path, gathered on
    the device; 0 where the path reaches a terminal without meeting a pour point; -100 on nodata and where the path
    enters a D8 cycle first.  Pour points on nodata cells are ignored."""
    f, p, d, pp = _checked(fdr, 1.0, dem, pour_points)
    H, W = f.shape
    lb = np.empty((H, W), np.int64)
    check(_lib.lib().dt_drainage(ptr(f, c_u8p), ptr(d, c_f32p), ptr(pp, c_i64p), H, W, p, None, None,
                                 ptr(lb, c_i64p)))
    return lb


def upslope_length(fdr, px=1.0, dem=None):
    """Upslope (longest) flow length (float64, TauDEM's plen): for every cell c, the length of the longest path that
    ends at c, the maximum over every cell s whose path passes through c (s = c included, so a source has 0).
    "Longest" is the exact order of n_card + n_diag * sqrt(2) on the integer move counts (two distinct count pairs
    never tie); the result is the length formula on the winning pair.  -100 on nodata and on cells of a D8 cycle;
    cells that drain into a cycle get their value."""
    f, p, d, _ = _checked(fdr, px, dem)
    H, W = f.shape
    out = np.empty((H, W), np.float64)
    check(_lib.lib().dt_upslope_length(ptr(f, c_u8p), ptr(d, c_f32p), H, W, p, ptr(out, c_f64p)))
    return out
