"""D8 flow direction (net-new): ESRI code of the neighbour that realises
slope.slope_gpu's maximum, first in its scan order NW,N,NE,W,E,SW,S,SE; 0 = nodata / interior
pit; a raster-border cell with no lower neighbour drains outward."""
import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_u8p, check, ptr


def d8(dem, px, return_slope=False, heights="float32"):
    """heights: "float32" (default) -- float32-exact heights only (ValueError otherwise); "float64" -- the
    differences taken in float64 (dt_d8_f64; slope as slope.sloper gives it on such a DEM); "auto" -- float64 exactly
    when float32 cannot hold the DEM (_lib.heights)."""
    d, wide = _lib.dem_tier(dem, heights)
    H, W = d.shape
    fdr = np.empty((H, W), np.uint8)
    sl = np.empty((H, W), np.float32) if return_slope else None
    if wide:
        check(_lib.lib().dt_d8_f64(ptr(d, c_f64p), H, W, float(px), ptr(fdr, c_u8p), ptr(sl, c_f32p)))
    else:
        check(_lib.lib().dt_d8_f32(ptr(d, c_f32p), H, W, float(px), ptr(fdr, c_u8p), ptr(sl, c_f32p)))
    return (fdr, sl) if return_slope else fdr


def d8_conditioned(dem, px, return_filled=False, heights="float32"):
    """D8 for DEMs with pits and flats (the reference takes such an `fdr` from a GIS tool,
    Example/example.py:36): depressions filled, D8 on the filled surface, flats routed to their nearest outlet
    (dt_d8_conditioned_f32).  Every valid cell gets a code; no cycles.
    heights: as in d8 -- "float32" (default) refuses heights float32 cannot hold; "float64" conditions in float64
    (dt_d8_conditioned_f64: the same definition, heights compared in float64; `filled` comes back as float64);
    "auto" -- float64 exactly when float32 cannot hold the DEM."""
    d, wide = _lib.dem_tier(dem, heights)
    H, W = d.shape
    fdr = np.empty((H, W), np.uint8)
    filled = np.empty((H, W), np.float64 if wide else np.float32) if return_filled else None
    info = np.zeros(3, np.int32)
    if wide:
        check(_lib.lib().dt_d8_conditioned_f64(ptr(d, c_f64p), H, W, float(px), ptr(fdr, c_u8p), ptr(filled, c_f64p),
                                               info.ctypes.data_as(_lib.c_i32p)))
    else:
        check(_lib.lib().dt_d8_conditioned_f32(ptr(d, c_f32p), H, W, float(px), ptr(fdr, c_u8p),
                                               ptr(filled, c_f32p), info.ctypes.data_as(_lib.c_i32p)))
    if info[0]:
        raise RuntimeError("%d flat cells could not be routed" % int(info[0]))
    return (fdr, filled) if return_filled else fdr


def d8_carved(dem, px, max_cut=None, return_filled=False):
    """Depression carving (Soille 2004; the complete form of breaching): (fdr, carved[, filled]).

    fdr and filled are d8_conditioned(dem, px, return_filled=True); lowest = flowpath.upslope_extreme(fdr, dem, "min",
    dem=dem).value, the lowest height at or above each cell on the conditioned D8 tree, which is non-increasing along
    every edge and <= dem.  max_cut None (or inf): carved = lowest -- every depression is cut open, nothing is raised.
    A finite max_cut >= 0: carved = maximum(lowest, filled - float32(max_cut)), both steps in float32: at most max_cut
    is cut and the rest filled (both terms are monotone along a path, so carved is too); max_cut=0 gives filled.
    Nodata cells (dem <= -100) keep their dem value.  HAND taken on `carved` along `fdr` is never negative, where the
    raw DEM along conditioned codes goes negative in every pit.
    The float32 tier only.  ValueError before any library call for heights float32 cannot hold, a NaN or +inf height,
    a px that is not finite and > 0, and a max_cut that is negative or NaN."""
    d = _args.raster(_lib.dem_f32(dem), "dem")
    p = _args.pixel_size(px)
    try:
        cut = float("inf") if max_cut is None else float(max_cut)
    except (TypeError, ValueError):
        cut = float("nan")
    if isinstance(max_cut, (bool, np.bool_)) or not cut >= 0:
        raise ValueError("max_cut must be a number >= 0 or None, not %r" % (max_cut,))
    if d.size and (np.isnan(d).any() or (d == np.inf).any()):
        raise ValueError("the DEM holds NaN or +inf heights, which conditioning does not take")
    H, W = d.shape
    fdr = np.empty((H, W), np.uint8)
    carved = np.empty((H, W), np.float32)
    filled = np.empty((H, W), np.float32) if return_filled else None
    info = np.zeros(3, np.int32)
    check(_lib.lib().dt_carve(ptr(d, c_f32p), H, W, p, cut, ptr(fdr, c_u8p), ptr(carved, c_f32p), ptr(filled, c_f32p),
                              info.ctypes.data_as(_lib.c_i32p)))
    if info[0]:
        raise RuntimeError("%d flat cells could not be routed" % int(info[0]))
    return (fdr, carved, filled) if return_filled else (fdr, carved)
