"""Flow-path extremes of a value raster on a D8 raster (net-new), on the GPU: the maximum or minimum of `values` over
everything upslope of a cell (TauDEM's D8FlowPathExtremeUp) or along its path downstream, optionally up to a stop mask.

Definition (the kernels in csrc/dt_flowpath.hip, the C header and the tests hold to it):

* Graph.  Exactly watershed.py's drainage graph: c -> succ(c) when c's code is one of the eight ESRI D8 codes, succ(c)
  lies in the raster and, when dem is given, neither cell is nodata (dem <= -100 in the DEM's own dtype).  A valid cell
  with no edge is a terminal.
* Values.  A float32 raster; any other real, integer or bool dtype is taken only when float32 holds every element
  exactly (ValueError otherwise, never a silent rounding).  NaN is "no value" and is skipped, -0.0 is taken as +0.0,
  +inf and -inf are ordinary values.  Nothing is added or rounded along a path: results are exact.
* Ties.  Between equal values the cell with the smallest flat index y * W + x holds the extreme.

Both functions give an Extreme(value, where): value float32, NaN on nodata and where there is no value; where int64, the
flat index of the cell that holds the extreme, -100 where value is NaN (None unless where=True).

Bad arguments raise ValueError before any library call: fdr that is not 2-D, dem / values / stop of another shape, a
kind other than "max" / "min", values float32 cannot hold, a stop of a float dtype, a raster of 2^31 cells or more.

Recipes (README.md): ridge height = upslope_extreme(fdr, dem, "max", dem).value - dem; barrier height =
downstream_extreme(fdr, dem, "max", dem).value - dem; flowdir.d8_carved is the upslope minimum of the DEM over the
conditioned codes.  Users of a resident chain call dt_dev_flowpath_upslope / dt_dev_flowpath_downstream on
chain.p("fdr")."""
from collections import namedtuple

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_i64p, c_u8p, check, nodata_mask, ptr

Extreme = namedtuple("Extreme", ["value", "where"])

_KIND = {"max": 0, "min": 1}


def _values_f32(values, shape):
    """values as a C-contiguous float32 raster; ValueError unless float32 holds every element (NaN included)"""
    a = _args.raster(values, "values", shape, "the direction raster", kinds="biuf")
    v = np.ascontiguousarray(a, np.float32)
    if a.dtype.type not in _lib._EXACT_IN_F32:
        k = _lib._first_inexact(a, v)
        if k >= 0:
            raise ValueError("values of dtype %s are not exactly representable in float32 (first at flat index %d: %r)"
                             % (a.dtype, k, a.reshape(-1)[k].item()))
    return v


def _checked(fdr, values, kind, dem, stop=None):
    f = _args.raster(fdr, "fdr", dtype=np.uint8)
    if not isinstance(kind, str) or kind not in _KIND:
        raise ValueError("kind must be \"max\" or \"min\", not %r" % (kind,))
    v = _values_f32(values, f.shape)
    d = nodata_mask(dem, f.shape)
    s = None
    if stop is not None:
        a = _args.raster(stop, "stop", f.shape, "the direction raster", kinds="biu")
        s = np.ascontiguousarray(a != 0, np.uint8)
    return f, v, _KIND[kind], d, s


def upslope_extreme(fdr, values, kind="max", dem=None, where=False):
    """Extreme(value, where) of `values` over everything upslope: for every cell c the max (kind="max") or min ("min")
    of values[s] over every valid cell s whose path contains c, s = c included.  A D8 cycle is no special case: a cell
    on a cycle gets the extreme over everything that reaches the cycle, the cycle included.  Cells with no value
    upstream and nodata cells get NaN (and -100 in where)."""
    f, v, k, d, _ = _checked(fdr, values, kind, dem)
    H, W = f.shape
    out = np.empty((H, W), np.float32)
    wh = np.empty((H, W), np.int64) if where else None
    check(_lib.lib().dt_flowpath_upslope(ptr(f, c_u8p), ptr(d, c_f32p), ptr(v, c_f32p), H, W, k, ptr(out, c_f32p),
                                         ptr(wh, c_i64p)))
    return Extreme(out, wh)


def downstream_extreme(fdr, values, kind="max", dem=None, stop=None, where=False):
    """Extreme(value, where) of `values` along the path downstream: the max / min over the cells of c's path, from c
    to where the path stops, both ends included.  stop=None: the path stops at its terminal; when it enters a D8 cycle
    the extreme is over its whole tail and the cycle.  stop given (an integer or bool raster, nonzero = stop; stop
    cells on nodata are ignored): the path stops at the first stop cell, c included, and a cell gets NaN / -100 where
    watershed.drainage with these pour points gives -100: where the path ends at a terminal, or runs round a cycle,
    without meeting a stop cell."""
    f, v, k, d, s = _checked(fdr, values, kind, dem, stop)
    H, W = f.shape
    out = np.empty((H, W), np.float32)
    wh = np.empty((H, W), np.int64) if where else None
    check(_lib.lib().dt_flowpath_downstream(ptr(f, c_u8p), ptr(d, c_f32p), ptr(v, c_f32p), ptr(s, c_u8p), H, W, k,
                                            ptr(out, c_f32p), ptr(wh, c_i64p)))
    return Extreme(out, wh)
