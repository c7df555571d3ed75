"""Greyscale geodesic reconstruction on the GPU (net-new; Vincent 1993): a marker raster spreads under a mask raster
until it stops.  One operator gives the four things the all-or-nothing depression tools (flowdir.d8_conditioned fills
everything, flowdir.d8_carved cuts everything open, filters.opening rounds off every ridge narrower than its window) do
not: fill only the noise (h-minima), say where the sinks and peaks are (regional extrema), fill towards chosen outlets
(seeded fill), and remove objects without rounding the terrain (opening / closing by reconstruction).

Definitions.  These are the contract; tests/_morphology_ref.py is their reference.

Valid cell.  The mask's height is finite and > -100.  Every other cell is nobody's neighbour and holds the no-value
marker (-100; 0 in a uint8 output) in every output.

Order.  Heights are compared by filters' order-preserving uint32 key of the float32 bits u: key = u ^ 0x80000000 when
the sign bit is clear, ~u when it is set (-0.0 below +0.0).  No valid or infinite float has key 0, nor does the
complement of its key, so 0 is free for "none".

Adjacency.  connectivity=8 (the default) or 4.

Given marker.  A user marker is given on a cell iff it is not NaN and > -100; +inf is allowed.  Otherwise the cell starts
from none.

Reconstruction by dilation.  F0(v) = min(marker(v), mask(v)) where the marker is given, else none.  R is the least
R >= F0 with R(v) = min(mask(v), max(R(v), max over the valid neighbours u of R(u))); equivalently R(v) is the maximum
over the paths from u to v of min(F0(u), the minimum of the mask along the path).

Reconstruction by erosion.  The dual: min and max swapped, and none is above everything.

Uniqueness.  The solution is unique, so it does not depend on schedule, tiling or run; a max-heap Dijkstra (widest path)
returns it.  It only selects among the input's float32 bit patterns, and is held bit for bit against that Dijkstra.

Erosion through dilation.  Erosion is dilation on complemented keys, ~R = dilate(~F, ~G): the device has one hot kernel,
which propagates a maximum of uint32 (csrc/dt_morphology.hip: 64 x 64 tiles on the tile-round schedule).

No value.  A valid cell that no marker reaches holds -100.

The functions take float32-exact DEMs (a DEM that float32 cannot hold raises ValueError, as in filters) and give float32
out.  Bad arguments raise ValueError before any library call: a raster that is not 2-D, shapes that differ, 2^31 cells or
more, a connectivity other than 4 or 8, an h that is not finite and > 0, a radius outside [1, 4096], a float raster as
`outlets`.  Empty rasters are allowed.  There is no CPU path.

Recipes.
    Depth in sink:            fill(dem) - dem                                    (on valid cells)
    Sink inventory:           zonal.statistics(regions.label(fill(dem) > dem), ...): area, depth, volume per sink
    Denoised conditioning:    flowdir.d8_conditioned(hminima(dem, 0.2), px)
    Object height (nDSM):     dem - opening_by_reconstruction(dem, R)
    Fill to the river or the sea only:  fill(dem, outlets=river == 1)"""
import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_i64p, c_u8p, check, ptr
from .device import host_empty

KINDS = ("dilation", "erosion")
RADIUS_MAX = 4096
# the marker modes of dt_morph_reconstruct (DT_MORPH_*)
_MARKER, _SHIFT, _STEP, _OUTLETS, _WINDOW = range(5)


class Reconstruction(np.ndarray):
    """the raster of a reconstruction.  `info`: the call's counts, {"rounds": rounds of tile visits that stored
    something, "changed": valid cells with R != F0, "tile_visits": visits of 64 x 64 tiles}"""
    info = None

    def __array_finalize__(self, obj):
        self.info = getattr(obj, "info", None)


def _with_info(r, info4):
    out = r.view(Reconstruction)
    out.info = {"rounds": int(info4[0]), "changed": int(info4[1]), "tile_visits": int(info4[2])}
    return out


def _f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a, np.float32)


def _call(mode, erosion, cn, mask, marker=None, seeds=None, h=0.0, radius=0, limit=0, u8=False):
    H, W = mask.shape
    out = host_empty((H, W), np.uint8 if u8 else np.float32)
    info = np.zeros(4, np.int64)
    check(_lib.lib().dt_morph_reconstruct(mode, int(erosion), cn, ptr(mask, c_f32p), ptr(marker, c_f32p),
                                          ptr(seeds, c_u8p), h, radius, H, W, limit,
                                          None if u8 else ptr(out, c_f32p), ptr(out, c_u8p) if u8 else None,
                                          ptr(info, c_i64p)))
    return _with_info(out, info)


def reconstruct(marker, mask, kind="dilation", connectivity=8, _visit_limit=0):
    """The reconstruction of `mask` (float32-exact heights) from `marker` (any real raster of the same shape, taken as
    float32) by `kind` ("dilation" or "erosion") -> Reconstruction (float32, -100 on invalid cells and where no marker
    reaches) with `.info`; the module docstring holds the definition.  `_visit_limit` (tests) caps the rounds of sweeps
    a workgroup makes per tile visit; the output does not depend on it."""
    g = _args.raster(mask, "mask")
    m = _args.raster(marker, "marker", shape=g.shape, other="mask", kinds="biuf")
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError("kind must be one of %s, not %r" % (KINDS, kind))
    cn = _args.connectivity(connectivity)
    limit = _args.integer(_visit_limit, "_visit_limit", 0, 2 ** 31 - 1)
    g = _lib.dem_f32(g, "mask")
    return _call(_MARKER, kind == "erosion", cn, g, marker=_f32(m), limit=limit)


def fill(dem, outlets=None, connectivity=8):
    """The depression fill of `dem` towards its outlets -> Reconstruction (float32): the reconstruction by erosion of the
    DEM from the marker that equals the DEM on the outlet cells and is none elsewhere, so every cell is raised to the
    lowest level from which it drains to an outlet.  outlets=None: the outlets are the valid cells on the raster's edge
    or with an invalid 8-neighbour -- the rule of flowdir.d8_conditioned, whose filled surface this equals on valid cells
    at connectivity 8.  `outlets` given (a bool / integer mask, != 0, regions' rule): only its valid cells are outlets; a
    one-cell void in a plain is then no outlet any more.  Cells that reach no outlet hold -100."""
    d = _args.raster(dem, "dem")
    seeds = None
    if outlets is not None:
        seeds = np.ascontiguousarray(_args.raster(outlets, "outlets", d.shape, "the DEM", kinds="biu") != 0, np.uint8)
    cn = _args.connectivity(connectivity)
    d = _lib.dem_f32(d)
    return _call(_OUTLETS, True, cn, d, seeds=seeds)


def _hextrema(dem, h, connectivity, erosion):
    d = _args.raster(dem, "dem")
    hh = _args.positive(h, "h")
    cn = _args.connectivity(connectivity)
    d = _lib.dem_f32(d)
    return _call(_SHIFT, erosion, cn, d, h=hh)


def hminima(dem, h, connectivity=8):
    """The h-minima transform -> Reconstruction (float32): the reconstruction by erosion of the DEM from the marker
    float32(float64(z) + h), h finite and > 0.  Depressions shallower than h disappear; deeper ones stay, shallower by
    h.  The marker is given on every valid cell, whatever its value, and is built on the device."""
    return _hextrema(dem, h, connectivity, True)


def hmaxima(dem, h, connectivity=8):
    """The h-maxima transform -> Reconstruction (float32): the reconstruction by dilation of the DEM from the marker
    max(float32(float64(z) - h), nextafter(float32(-100), +inf)).  Peaks lower than h disappear; higher ones stay, lower
    by h.  The clamp keeps the result a valid height; it changes only cells within h of -100."""
    return _hextrema(dem, h, connectivity, False)


def _regional(dem, connectivity, erosion):
    d = _args.raster(dem, "dem")
    cn = _args.connectivity(connectivity)
    d = _lib.dem_f32(d)
    return np.asarray(_call(_STEP, erosion, cn, d, u8=True))


def regional_minima(dem, connectivity=8):
    """uint8 raster: 1 on the cells of the plateaus (connected cells of one key) that have no strictly lower valid
    neighbour, 0 elsewhere and on invalid cells.  Computed as R != dem, R the reconstruction by erosion from the marker
    whose key is the DEM's key + 1.  The raster's edge is not a neighbour: a plateau on the edge with no lower
    neighbour inside the raster is a minimum."""
    return _regional(dem, connectivity, True)


def regional_maxima(dem, connectivity=8):
    """uint8 raster: 1 on the cells of the plateaus that have no strictly higher valid neighbour, 0 elsewhere and on
    invalid cells (reconstruction by dilation from the key - 1).  The raster's edge is not a neighbour."""
    return _regional(dem, connectivity, False)


def _by_reconstruction(dem, radius, connectivity, erosion):
    d = _args.raster(dem, "dem")
    r = _args.integer(radius, "radius", 1, RADIUS_MAX)
    cn = _args.connectivity(connectivity)
    d = _lib.dem_f32(d)
    return _call(_WINDOW, erosion, cn, d, radius=r)


def opening_by_reconstruction(dem, radius, connectivity=8):
    """Opening by reconstruction -> Reconstruction (float32): the reconstruction by dilation under the DEM of the marker
    filters.minimum(dem, radius) (radius an integer in [1, 4096]).  What the window minimum removed and cannot be
    reached again -- objects narrower than the window -- stays removed; everything else comes back bit for bit.  One
    library call: the window pass and the reconstruction stay on the device."""
    return _by_reconstruction(dem, radius, connectivity, False)


def closing_by_reconstruction(dem, radius, connectivity=8):
    """Closing by reconstruction -> Reconstruction (float32): the reconstruction by erosion of the marker
    filters.maximum(dem, radius); pits narrower than the window are closed, everything else keeps its bits."""
    return _by_reconstruction(dem, radius, connectivity, True)
