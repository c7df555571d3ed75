"""DEM filters (net-new): the minimum, maximum and range of a window at any radius with morphological opening and
closing, the window percentile (median), and feature-preserving denoising (Sun et al. 2007, as used for DEMs by Lindsay
et al. 2019).  Recipes: range is local relief; opening removes off-terrain objects, bridges and decks before
flowdir.d8_conditioned; closing and opening tidy a binary flood map; dem - minimum(dem, R) is a height above the local
floor that needs no flow directions; median despeckles; denoise takes the LiDAR noise out of D8, HAND, slope and
curvature and keeps the banks and levees a mean filter removes.

Validity.  A height is valid iff it is finite and > -100, as everywhere in the package.

Window.  The window of radius R around (y, x) is the (2 R + 1)^2 square clipped to the raster; invalid cells inside it
are skipped.  A cell HAS A VALUE iff its own height is valid (focal's rule); the no-value marker is -100.

Order.  Heights are compared by the order-preserving integer key of their float32 bits u: key = u ^ 0x80000000 when the
sign bit is clear, ~u when it is set.  On valid heights that is the order of the reals, with -0.0 below +0.0, so every
extreme and every rank is the bit pattern of one particular height of the window.

1. Extremes (radius in [1, 4096]).  min and max are the smallest and the largest valid height of the window; range =
float32(float64(max) - float64(min)).  opening is the maximum of the minimum raster and closing the minimum of the
maximum raster: the second pass runs on the first pass's raster, whose no-value cells are invalid, so the validity mask
of both passes is the input's.  The cost per cell does not depend on the radius (running extremes over segments of
2 R + 1 cells along the rows, then along the columns).  morphology.opening_by_reconstruction / closing_by_reconstruction
are the forms that remove the same objects and give every other cell back bit for bit.

2. Percentile (radius in [1, 16], q finite and in [0, 100]).  With n the number of valid cells of the window, the output
is the element of index
    k(n) = min(n - 1, int(floor(q / 100.0 * (n - 1) + 0.5)))            (Python float64; k(0) = 0)
of the window's valid heights sorted ascending by key: always one of the window's heights, never an average.
rank_table(radius, q) is k(0 .. (2 R + 1)^2) as uint16; the host computes it once and the device looks it up.

3. Denoise (radius in [1, 16], threshold in degrees in (0, 90), iterations in [1, 32], max_change > 0 and finite, px the
cell size).  t = math.cos(math.radians(threshold)), on the host.  All arithmetic is IEEE float64 on the float32 heights,
only + - * / sqrt, in exactly this association; x points east (columns), y south (rows).
  Normals.  For a valid cell z_c, each of its eight neighbours is its height when it is on the raster and valid, else
    2.0 * z_c - z_opposite  when the opposite neighbour is valid, else z_c.
    gx = ((NE + 2.0 * E) + SE) - ((NW + 2.0 * W) + SW)        gy = ((SW + 2.0 * S) + SE) - ((NW + 2.0 * N) + NE)
    n = (-gx, -gy, 8.0 * px)        l = sqrt((nx * nx + ny * ny) + nz * nz)        n^ = float32(n / l), per component
  Smoothed normals.  Over the valid cells i of the clipped window in row-major order (the centre included), on the
    float32 unit normals:  c = (xc * xi + yc * yi) + zc * zi;  where c > t:  w = (c - t) * (c - t) and
    m = m + w * n^_i, per component.  l = sqrt((mx * mx + my * my) + mz * mz),  m^ = float32(m / l), per component.
  Update, `iterations` Jacobi steps from the input heights z0.  For a valid cell, over its valid neighbours i on the
    raster in the order E, SE, S, SW, W, NW, N, NE at offset (dx, dy), with (a, b, c) the smoothed normal:
    d = (ac * ai + bc * bi) + cc * ci;  where d > t:  w = (d - t) * (d - t),
    e = z_i + (ai * (dx * px) + bi * (dy * px)) / ci,  sw = sw + w,  sz = sz + w * e.
    With sw > 0:  z^ = float32(sz / sw), and z^ replaces the height iff |float64(z^) - float64(z0)| <= max_change;
    otherwise the previous iterate stays.  Invalid cells keep the input's bits.

Every output equals the numpy reference of the test suite bit for bit."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_u16p, check, ptr

OUTPUTS = ("min", "max", "range")
RADIUS_MAX = 4096
RANK_RADIUS_MAX = 16
DENOISE_RADIUS_MAX = 16
ITERATIONS_MAX = 32
_C_NAMES = ("min", "max", "range", "opening", "closing")


def _outputs(outputs):
    if isinstance(outputs, str) or not hasattr(outputs, "__iter__"):
        raise ValueError("outputs must be a sequence of names from %s, not %r" % (OUTPUTS, outputs))
    names = tuple(outputs)
    if not names:
        raise ValueError("outputs is empty; name at least one of %s" % (OUTPUTS,))
    for n in names:
        if not isinstance(n, str) or n not in OUTPUTS:
            raise ValueError("output %r is not one of %s" % (n, OUTPUTS))
    if len(set(names)) != len(names):
        raise ValueError("outputs names an output twice: %r" % (names,))
    return names


def _real(v, what, lo, hi, closed):
    """v as a float; ValueError unless it is a number (not a bool) in [lo, hi] (closed) or (lo, hi)"""
    try:
        f = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not (lo <= f <= hi if closed else lo < f < hi):
        raise ValueError("%s must be a number in %s%g, %g%s, not %r" % (what, "[" if closed else "(", lo, hi,
                                                                        "]" if closed else ")", v))
    return f


def _call_extremes(dem, radius, names):
    d = _args.raster(dem, "dem")
    r = _args.integer(radius, "radius", 1, RADIUS_MAX)
    d = _lib.dem_f32(d)
    H, W = d.shape
    out = {n: np.empty(d.shape, np.float32) for n in names}
    check(_lib.lib().dt_filter_extremes(ptr(d, c_f32p), H, W, r, *(ptr(out.get(n), c_f32p) for n in _C_NAMES)))
    return out


def extremes(dem, radius, outputs=("min", "max")):
    """The window extremes named in `outputs` (any of OUTPUTS, each once) of `dem` (float32-exact heights; a DEM that
    float32 cannot hold raises ValueError) over the window of `radius` (an integer in [1, 4096]) -> dict {name:
    float32 raster[H, W]} in the order asked for; -100 where there is no value.  The module docstring holds the
    definition.  The cost per cell does not depend on the radius.  Bad arguments raise ValueError before any library
    call."""
    names = _outputs(outputs)
    return _call_extremes(dem, radius, names)


def minimum(dem, radius):
    """extremes' min alone: the smallest valid height of the window (erosion)"""
    return _call_extremes(dem, radius, ("min",))["min"]


def maximum(dem, radius):
    """extremes' max alone: the largest valid height of the window (dilation)"""
    return _call_extremes(dem, radius, ("max",))["max"]


def relief(dem, radius):
    """extremes' range alone: float32(float64(max) - float64(min)), the local relief"""
    return _call_extremes(dem, radius, ("range",))["range"]


def opening(dem, radius):
    """The morphological opening: the window maximum of the window minimum, one library call (the intermediate raster
    stays on the device)"""
    return _call_extremes(dem, radius, ("opening",))["opening"]


def closing(dem, radius):
    """The morphological closing: the window minimum of the window maximum, one library call"""
    return _call_extremes(dem, radius, ("closing",))["closing"]


def rank_table(radius, q):
    """k(0 .. (2 radius + 1)^2) of the module docstring as a uint16 array: the index of the output among the n valid
    heights of a window, sorted ascending"""
    r = _args.integer(radius, "radius", 1, RANK_RADIUS_MAX)
    f = _real(q, "q", 0.0, 100.0, True)
    cells = (2 * r + 1) ** 2
    k = [0] + [min(n - 1, int(math.floor(f / 100.0 * (n - 1) + 0.5))) for n in range(1, cells + 1)]
    return np.asarray(k, np.uint16)


def percentile(dem, radius, q=50.0):
    """The height at percentile `q` (finite, in [0, 100]) of the valid heights of the window of `radius` (an integer in
    [1, 16]) of `dem` (float32-exact heights) -> float32 raster[H, W], -100 where there is no value: element k(n) of the
    n heights sorted ascending (module docstring), always one of the window's heights.  q = 0 is the minimum, 100 the
    maximum.  Bad arguments raise ValueError before any library call."""
    d = _args.raster(dem, "dem")
    table = rank_table(radius, q)
    d = _lib.dem_f32(d)
    H, W = d.shape
    out = np.empty(d.shape, np.float32)
    check(_lib.lib().dt_filter_rank(ptr(d, c_f32p), H, W, int(radius), ptr(table, c_u16p), table.size,
                                    ptr(out, c_f32p)))
    return out


def median(dem, radius):
    """percentile at q = 50: the despeckling filter (with an even count, the upper of the two middle heights)"""
    return percentile(dem, radius, 50.0)


def denoise(dem, px, radius=5, threshold=15.0, iterations=3, max_change=0.5):
    """Feature-preserving denoising of `dem` (float32-exact heights, cell size `px`) -> float32 raster[H, W]: the
    normals are smoothed over the window of `radius` (an integer in [1, 16]) among the cells whose normal lies within
    `threshold` degrees (in (0, 90)) of the centre's, then `iterations` (an integer in [1, 32]) steps pull the heights
    towards the smoothed facets of their neighbours; no height moves more than `max_change` (> 0, metres) from the
    input.  Invalid cells come back bit-identical.  The module docstring holds the definition.  Bad arguments raise
    ValueError before any library call."""
    d = _args.raster(dem, "dem")
    p = _args.pixel_size(px)
    r = _args.integer(radius, "radius", 1, DENOISE_RADIUS_MAX)
    th = _real(threshold, "threshold", 0.0, 90.0, False)
    it = _args.integer(iterations, "iterations", 1, ITERATIONS_MAX)
    mc = _args.positive(max_change, "max_change")
    d = _lib.dem_f32(d)
    t = math.cos(math.radians(th))
    if not 0.0 < t < 1.0:
        raise ValueError("threshold=%r has no cosine strictly between 0 and 1" % (threshold,))
    H, W = d.shape
    out = np.empty(d.shape, np.float32)
    check(_lib.lib().dt_filter_denoise(ptr(d, c_f32p), H, W, p, r, t, it, mc, ptr(out, c_f32p)))
    return out
