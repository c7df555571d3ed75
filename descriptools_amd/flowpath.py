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
chain.p("fdr").

Weighted flow-path sums (net-new): downstream_sum, the sum of a per-cell cost along a cell's own path, and
upslope_longest, the longest such sum that ends at a cell; with the cost step length / velocity they are travel_time
(to the outlet, or to the channel with stop=river) and time_of_concentration.  Definition (the k_ps_* kernels, the C
header and tests/_pathsum_ref.py hold to it):

* Graph.  The one above.
* Weights.  Validated as flowacc.accumulate_weighted validates them: a real or integer dtype, finite, >= 0.  Quantised
  as q(c) = rint(w(c) * 2^s), round half to even, s = frac_bits, by default path_frac_bits(weights): the finest s with
  N * rint(max(weights) * 2^s) <= 2^52, accumulate_weighted's rule.  A path has fewer than N moves, so every sum is at
  most 2^52 and converts to float64 exactly: the results are exact sums of the quantised weights, independent of
  order, tiling and run.  q(c) is the cost of the move out of c; the weight of the cell where a path stops is never
  counted.
* Downstream sum.  T(target) = 0 and T(c) = q(c) + T(succ(c)).  The target is the path's terminal; with `stop` it is
  the first stop cell on the path, c included (stop cells on nodata are ignored).  The output is float64 T * 2^-s, and
  -100 exactly where watershed.drainage(fdr, dem=dem, pour_points=stop) gives -100: on nodata, where the path enters a
  D8 cycle before it stops, and (with stop) where it reaches a terminal without meeting a stop cell.
* Upslope longest.  U(c) = the max over every cell s whose path contains c (s = c included) of the sum of q over the
  cells of s's path from s up to but excluding c; a source has 0.  It is -100 wherever the stop-less T(c) is -100:
  on nodata, on a D8 cycle and on every cell that drains into one.  This is wider than watershed.upslope_length's
  rule, which keeps the cells that drain into a cycle.  For every s upslope of c, T(s) = D(s -> c) + T(c), so
  U(c) = M(c) - T(c) with M the maximum of T over everything upslope of c: that is how it is computed, and why the cell
  that holds the longest path (a `where`) is not offered -- the 64-bit key of the fold is all sum.

Bad arguments of these raise ValueError before any library call as well: a wrong shape, a float stop, a non-integer
frac_bits or one that is too fine, weights that are negative or not finite, a speed that is not finite and > 0 on a
valid non-terminal cell, 2^31 cells or more.  Users of a resident chain call dt_dev_flowpath_downstream_sum /
dt_dev_flowpath_upslope_longest on chain.p("fdr"); README.md has the recipes: isochrones and
time-area curves with zonal.histogram, a unit hydrograph for inundation.simulate, hillslope travel time to the channel,
mean slope along the path."""
from collections import namedtuple

import numpy as np

from . import _args, _lib, flowacc
from ._lib import c_f32p, c_f64p, c_i64p, c_u8p, check, nodata_mask, ptr

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


# ---- weighted flow-path sums ----------------------------------------------------------------------------------------
_CARDINAL = (1, 4, 16, 64)
_DIAGONAL = (2, 8, 32, 128)
_DELTA = {1: (0, 1), 2: (1, 1), 4: (1, 0), 8: (1, -1), 16: (0, -1), 32: (-1, -1), 64: (-1, 0), 128: (-1, 1)}


def _stop_u8(stop, shape):
    if stop is None:
        return None
    a = _args.raster(stop, "stop", shape, "the direction raster", kinds="biu")
    return np.ascontiguousarray(a != 0, np.uint8)


def _sum_args(fdr, weights, dem, stop, frac_bits):
    f = _args.raster(fdr, "fdr", dtype=np.uint8)
    w = flowacc._weights_f64(weights, f.shape)
    d = nodata_mask(dem, f.shape)
    st = _stop_u8(stop, f.shape)
    n = f.size
    s = _args.frac_bits(n, float(w.max()) if n else 0.0, frac_bits,
                        " for these weights: N * rint(max(weights) * 2^frac_bits)", "path_frac_bits gives")
    return f, w, d, st, s


def path_frac_bits(weights):
    """The fixed-point scale downstream_sum and upslope_longest use by default, flowacc.weight_frac_bits's: the largest
    s with N * rint(max(weights) * 2^s) <= 2^52 over the raster's N cells.  All-zero weights and an empty raster give
    0.  The weights are validated as the two functions validate them."""
    return flowacc.weight_frac_bits(weights)


def downstream_sum(fdr, weights, dem=None, stop=None, frac_bits=None):
    """float64 T * 2^-s: the sum of the quantised weights q = rint(weights * 2^s) over the moves of each cell's path,
    from the cell down to the path's terminal or, with `stop` (an integer or bool raster, nonzero = stop), to the first
    stop cell on it, the cell itself included.  weights[c] is the cost of the move out of c; the weight of the cell
    where the path stops is not counted, so a target has 0.  -100 exactly where watershed.drainage(fdr, dem=dem,
    pour_points=stop) gives -100: on nodata, where the path enters a D8 cycle before it stops, and (with stop) where
    it reaches a terminal without meeting a stop cell.  s = frac_bits, by default path_frac_bits(weights); pass
    frac_bits=0 for integer weights to get exact integer sums (weights of 1: the number of moves)."""
    f, w, d, st, s = _sum_args(fdr, weights, dem, stop, frac_bits)
    H, W = f.shape
    out = np.empty((H, W), np.float64)
    check(_lib.lib().dt_flowpath_downstream_sum(ptr(f, c_u8p), ptr(d, c_f32p), ptr(w, c_f64p), ptr(st, c_u8p), H, W, s,
                                                ptr(out, c_f64p)))
    return out


def upslope_longest(fdr, weights, dem=None, frac_bits=None):
    """float64 U * 2^-s: for every cell c the largest, over every cell s whose path contains c (s = c included), of
    the sum of the quantised weights over the cells of s's path from s up to but excluding c -- the cost of the longest
    path that ends at c.  A source has 0.  -100 wherever the stop-less downstream_sum is -100: on nodata, on a D8 cycle
    and on every cell that drains into one (watershed.upslope_length keeps the latter; this does not, because a cell
    without a downstream sum has no place in U = M - T).  frac_bits as in downstream_sum."""
    f, w, d, _, s = _sum_args(fdr, weights, dem, None, frac_bits)
    H, W = f.shape
    out = np.empty((H, W), np.float64)
    check(_lib.lib().dt_flowpath_upslope_longest(ptr(f, c_u8p), ptr(d, c_f32p), ptr(w, c_f64p), H, W, s,
                                                 ptr(out, c_f64p)))
    return out


def _moves(f, d):
    """(has an edge, the edge is diagonal) per cell of the drainage graph; plain numpy"""
    H, W = f.shape
    valid = np.ones((H, W), bool) if d is None else ~(d <= -100)
    yy, xx = np.indices((H, W))
    edge = np.zeros((H, W), bool)
    for code, (dy, dx) in _DELTA.items():
        m = (f == code) & valid
        ty, tx = yy[m] + dy, xx[m] + dx
        ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        ok[ok] = valid[ty[ok], tx[ok]]
        edge[yy[m][ok], xx[m][ok]] = True
    return edge, edge & np.isin(f, _DIAGONAL)


def step_length(fdr, px, dem=None):
    """float64 length of the move out of each cell on the drainage graph: px on a cardinal code, px * sqrt(2.0) on a
    diagonal one, 0 on terminals and nodata.  Plain numpy."""
    f = _args.raster(fdr, "fdr", dtype=np.uint8)
    p = _args.pixel_size(px)
    edge, diag = _moves(f, nodata_mask(dem, f.shape))
    return np.where(diag, p * np.sqrt(2.0), np.where(edge, p, 0.0))


def _time_weights(fdr, px, speed, dem):
    """step_length / speed on the cells that have a move, 0 elsewhere (where speed is not looked at)"""
    f = _args.raster(fdr, "fdr", dtype=np.uint8)
    step = step_length(f, px, dem)
    v = _args.raster(speed, "speed", f.shape, "the direction raster", kinds="biuf")
    moving = step > 0
    vm = np.asarray(v[moving], np.float64)
    bad = ~(np.isfinite(vm) & (vm > 0))
    if bad.any():
        k = int(np.flatnonzero(moving.reshape(-1))[np.argmax(bad)])
        raise ValueError("speed must be finite and > 0 on every valid cell that has a move (first at flat index %d: %r)"
                         % (k, v.reshape(-1)[k].item()))
    w = np.zeros(f.shape, np.float64)
    w[moving] = step[moving] / vm
    return f, w


def travel_time(fdr, px, speed, dem=None, stop=None, frac_bits=None):
    """downstream_sum(fdr, step_length(fdr, px, dem) / speed, dem, stop, frac_bits): the time along each cell's path to
    its outlet or, with stop=river, to the channel, for a speed raster in px's length unit per time unit.  speed must
    be finite and > 0 on every valid non-terminal cell (ValueError naming the first offender); elsewhere it is not
    looked at."""
    f, w = _time_weights(fdr, px, speed, dem)
    return downstream_sum(f, w, dem, stop, frac_bits)


def time_of_concentration(fdr, px, speed, dem=None, frac_bits=None):
    """upslope_longest(fdr, step_length(fdr, px, dem) / speed, dem, frac_bits): the longest travel time from anywhere
    upslope to each cell.  speed as in travel_time."""
    f, w = _time_weights(fdr, px, speed, dem)
    return upslope_longest(f, w, dem, frac_bits)
