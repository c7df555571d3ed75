"""Multi-resolution valley bottom flatness MRVBF and ridge top flatness MRRTF (net-new; Gallant & Dowling 2003, Water
Resources Research 39(12)): how flat and how low (MRVBF) or how flat and how high (MRRTF) a cell lies, judged at a
sequence of scales that coarsen by three, combined so that the coarsest scale at which a cell still counts as a flat
valley bottom (ridge top) decides the integer part of its value.  It needs no flow direction, so it holds on
unconditioned DEMs, coastal plains and wide floodplains; values above about 0.5 .. 1.5 mark depositional flats, and the
raster goes into evaluation.calibration and evaluation.curve with 'over'.  Its two building blocks are ops of their own:
the elevation percentile of a disc (Lindsay's EP) and one generalisation step.

Validity.  A height is valid iff it is finite and > -100.  All arithmetic is IEEE float64 on the float32 heights in
exactly the association given; the rasters a pyramid level keeps are rounded to float32.

N(x, t, p) = 1 / (1 + (x / t)^p); with q = x / t the power is q q q for p = 3, (q q) (q q) for p = 4 and pow(q, p)
otherwise.

Slope (percent) of a surface z of cell size c at a valid cell.  Per axis (z+ - z-) / (2 c) when both neighbours are
valid and inside the raster, (z+ - z) / c or (z - z-) / c when only one is, 0 when neither is; with p along the columns
and q along the rows, S = 100 sqrt(p p + q q).

Percentile at radius r.  Over the disc dx^2 + dy^2 <= r^2 clipped to the raster, centre included: n valid cells, l of
them with z < z_c and h with z > z_c, compared as float32.  lower = l / n, higher = h / n; a value exists iff the centre
is valid.

Coarsen a raster of cell size c.  Weights g[k] = exp(-k^2 / 18), k = 0..5 (sigma = 3 cells, 11 x 11), computed on the
host.  num = the row sums of g z over the valid cells, k ascending -5..5, then the column sums of those, again
ascending; den the same of g [valid].  The smoothed height of a valid cell is num / den; the slope of the smoothed
surface is taken at cell size c, a neighbour counting where its own height is valid.  Coarse cell (I, J) is the mean of
the smoothed height, and of the slope, over the valid cells of the fine rows 3I..3I+2 and columns 3J..3J+2 (clipped to
the raster), summed in row-major order, divided by the count and rounded to float32; -100 when the block has no valid
cell.  The next level's cell size is 3 c.

Levels.  Levels 1 and 2 are the base raster, level L >= 3 is the base raster coarsened L - 2 times.  default_levels is
the largest L <= 10 whose level-L grid (ceiling division by 3, L - 2 times) still has at least 4 cells on its shorter
side, never less than 2.  An explicit `levels` is taken as given: grids may shrink to a single cell.

Interpolation of a level-L raster to base cell (y, x), s = 3^(L-2).  Per axis a = 2 y + 1 - s, i0 = floor(a / (2 s)),
f = (a - i0 2 s) / (2 s); when i0 < 0 or i0 >= n_c - 1, i0 is clamped into [0, n_c - 1] and f = 0; i1 = min(i0 + 1,
n_c - 1).  The four corners in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1) with the weights wy wx, wy = 1 - fy
and fy, wx = 1 - fx and fx; corners holding -100 are skipped; the value is sum(w c) / sum(w), and the coarse cell
(y // s, x // s) when sum(w) is 0.

Index.  With t = slope_threshold, t_L = t / 2^(L-1) and p_L = log10((L - 0.5) / 0.1) / log10(1.5) (host math):
    level 1, P the radius-3 percentile, unrounded      VF_1 = 1 - N(N(S_1, t_1, 4) N(P, T, 3), 0.3, 4)
    level 2, P the radius-6 percentile, unrounded      CF_2 = N(S_1, t_2, 4)
                                                       VF_2 = 1 - N(CF_2 N(P, T, 3), 0.3, 4)
                                                       W_2 = 1 - N(VF_2, 0.4, p_2)
                                                       M_2 = W_2 (1 + VF_2) + (1 - W_2) VF_1
    level L >= 3, S_L and P_L the interpolated float32 slope and radius-6 percentile of that level
                                                       CF_L = CF_(L-1) N(S_L, t_L, 4)
                                                       VF_L = 1 - N(CF_L N(P_L, T, 3), 0.3, 4)
                                                       W_L = 1 - N(VF_L, 0.4, p_L)
                                                       M_L = W_L (L - 1 + VF_L) + (1 - W_L) M_(L-1)
mrvbf takes the lower percentile and T = pctl_valley, mrrtf the higher percentile and T = pctl_ridge; slopes and the
pyramid are shared.  The output is float32(M_levels) on valid cells and -100 elsewhere.

elevation_percentile and coarsen equal the numpy reference of the test suite bit for bit.  indices takes one pow per
level and output; tests/test_gpu_mrvbf.py derives and states its tolerance."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, check, ptr

OUTPUTS = ("mrvbf", "mrrtf")
LEVELS_MAX = 10
PERCENTILE_RADIUS_MAX = 16
_KINDS = ("lower", "higher")


def _first_threshold(p):
    return 16.0 * (25.0 / p) ** (math.log(2.0) / math.log(3.0))


def slope_threshold(px):
    """The first slope threshold in percent at pixel size `px`: 16 % at 25 m, doubled for every factor three of finer
    resolution (Gallant & Dowling 2003): 16 (25 / px)^(ln 2 / ln 3)"""
    return _first_threshold(_args.pixel_size(px))


def default_levels(shape):
    """The largest L <= LEVELS_MAX whose level-L grid (ceiling division of `shape` by 3, L - 2 times) still has at
    least 4 cells on its shorter side; never less than 2"""
    h, w = (_args.integer(n, "a shape entry", 0) for n in shape)
    best = 2
    for L in range(3, LEVELS_MAX + 1):
        h, w = -(-h // 3), -(-w // 3)
        if min(h, w) < 4:
            break
        best = L
    return best


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


def _real(v, what, ok, bound):
    try:
        f = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not (math.isfinite(f) and ok(f)):
        raise ValueError("%s must be a finite number %s, not %r" % (what, bound, v))
    return f


def _exponents(levels):
    """p_L of the levels 2 .. levels"""
    return np.array([math.log10((L - 0.5) / 0.1) / math.log10(1.5) for L in range(2, levels + 1)], np.float64)


def _gauss_weights():
    return np.array([math.exp(-(k * k) / 18.0) for k in range(6)], np.float64)


def indices(dem, px, outputs=("mrvbf",), slope_threshold=None, levels=None, pctl_valley=0.4, pctl_ridge=0.35):
    """The indices named in `outputs` (any of OUTPUTS, each once) of `dem` (float32-exact heights; a DEM that float32
    cannot hold raises ValueError, as terrain.attributes does) at pixel size `px` -> dict {name: float32 raster[H, W]}
    in the order asked for, -100 where the height is not valid.  The module docstring holds the definition.
    slope_threshold (percent, finite and > 0) defaults to slope_threshold(px), levels (an integer in [2, 10]) to
    default_levels(dem.shape); pctl_valley and pctl_ridge lie in (0, 1].  Only what is asked for is computed.  Bad
    arguments raise ValueError before any library call."""
    d = _args.raster(dem, "dem")
    p = _args.pixel_size(px)
    names = _outputs(outputs)
    t = _first_threshold(p) if slope_threshold is None else _real(slope_threshold, "slope_threshold", lambda f: f > 0,
                                                                  "> 0")
    L = default_levels(d.shape) if levels is None else _args.integer(levels, "levels", 2, LEVELS_MAX)
    Tv = _real(pctl_valley, "pctl_valley", lambda f: 0 < f <= 1, "in (0, 1]")
    Tr = _real(pctl_ridge, "pctl_ridge", lambda f: 0 < f <= 1, "in (0, 1]")
    d = _lib.dem_f32(d)
    out = {n: np.empty(d.shape, np.float32) for n in names}
    H, W = d.shape
    pL = _exponents(L)
    check(_lib.lib().dt_mrvbf(ptr(d, c_f32p), H, W, p, t, L, Tv, Tr, ptr(pL, c_f64p), ptr(out.get("mrvbf"), c_f32p),
                              ptr(out.get("mrrtf"), c_f32p)))
    return out


def mrvbf(dem, px, slope_threshold=None, levels=None, pctl_valley=0.4):
    """indices' mrvbf alone: the valley bottom flatness, float32, -100 where the height is not valid"""
    return indices(dem, px, ("mrvbf",), slope_threshold, levels, pctl_valley=pctl_valley)["mrvbf"]


def mrrtf(dem, px, slope_threshold=None, levels=None, pctl_ridge=0.35):
    """indices' mrrtf alone: the ridge top flatness, float32, -100 where the height is not valid"""
    return indices(dem, px, ("mrrtf",), slope_threshold, levels, pctl_ridge=pctl_ridge)["mrrtf"]


def elevation_percentile(dem, radius, kind="lower"):
    """The share of the valid cells of the disc of `radius` (an integer in [1, 16]) around every cell that lie strictly
    lower (kind 'lower': 0 in a pit, near 1 on a peak) or strictly higher (kind 'higher') than the cell -> float32
    raster, -100 where the height is not valid"""
    d = _args.raster(dem, "dem")
    r = _args.integer(radius, "radius", 1, PERCENTILE_RADIUS_MAX)
    if not isinstance(kind, str) or kind not in _KINDS:
        raise ValueError("kind must be one of %s, not %r" % (_KINDS, kind))
    d = _lib.dem_f32(d)
    out = np.empty(d.shape, np.float32)
    H, W = d.shape
    lo, hi = (out, None) if kind == "lower" else (None, out)
    check(_lib.lib().dt_percentile(ptr(d, c_f32p), H, W, r, ptr(lo, c_f32p), ptr(hi, c_f32p)))
    return out


def coarsen(dem, px):
    """One generalisation step of `dem` at pixel size `px` -> (dem3, slope3): the Gaussian-smoothed heights and the
    slope of the smoothed surface in percent, both as 3 x 3 block means at pixel size 3 px, float32 rasters of shape
    (ceil(H / 3), ceil(W / 3)), -100 where the block has no valid cell"""
    d = _args.raster(dem, "dem")
    p = _args.pixel_size(px)
    d = _lib.dem_f32(d)
    H, W = d.shape
    shape3 = (-(-H // 3), -(-W // 3))
    dem3, slope3 = np.empty(shape3, np.float32), np.empty(shape3, np.float32)
    g = _gauss_weights()
    check(_lib.lib().dt_coarsen(ptr(d, c_f32p), H, W, p, ptr(g, c_f64p), ptr(dem3, c_f32p), ptr(slope3, c_f32p)))
    return dem3, slope3
