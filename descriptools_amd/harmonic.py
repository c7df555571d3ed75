"""Harmonic interpolation on a masked raster (net-new): the discrete harmonic function with some cells held fixed and
zero flux at nodata and at the raster's edge -- what fills the voids of a LiDAR or SRTM DEM (GDAL's fillnodata, SAGA's
"Close Gaps"), and what SAGA's "Channel Network Base Level" interpolates: the surface through the river cells' heights,
whose difference to the DEM is the vertical distance to channel network (VDCN), the alternative to HAND where the D8
staircase or the choice of one nearest river cell shows as seams.  The same surface through ridge cells gives valley
depth and the normalised height.

Inputs.  `values`: a 2-D real raster, taken as float32 and widened to float64.  `fixed`: the same shape, taken as int8;
a cell is fixed iff fixed == 1 and its value is finite.  `domain`: the same shape, a cell is in it iff domain != 0, or
None for everywhere.  A fixed cell is always in the domain.  A cell with fixed == 1 and a non-finite value (NaN, +-inf)
is outside the domain.  The values of free cells are never read.  A value at or below the -100 sentinel is a number like
any other here; base_level, vdcn and fill_voids take the DEM's nodata cells (_lib.nodata_mask) out of the domain.

Equation.  On every free cell v of the domain that has k >= 1 of its four edge neighbours (N, W, E, S) in the domain:
s = the sum of those neighbours' u, in that order, left to right, one rounding per addition; avg = s / k in float64,
one division; r(v) = |avg - u(v)|.  u solves r = 0; fixed cells hold their value.  Connectivity is 4.

Components.  Free cells that no 4-connected path through the domain joins to a fixed cell have no value: interpolate
removes them with regions.connected(domain, fixed, connectivity=4) before the library call and counts them as
`unreached`.  (The C entries state this as a precondition; without it such cells settle on an unspecified constant.)

What a call returns.  A field whose fixed cells carry their input value exactly and whose residual r, evaluated with
exactly the expression above, is <= tol at every solved cell -- or RuntimeError when the budget of rounds ran out first.
It is the same bits on every run with the same inputs: coloured rounds of tile visits, red-black sweeps with a barrier
between the half-sweeps, no float atomics.  The iterate at which the residual test passes depends on the schedule
(csrc/dt_harmonic.hip: tiles of 64 x 64, 4 over-relaxed red-black sweeps per visit, a pyramid by 2 solved from the
coarsest level up, each level starting from the one below by injection), so equality with another solver is NOT part of
the contract.  A field with r <= tol differs from the exact solution by at most tol * max(t), t the expected hitting
time of the fixed cells by the random walk on the domain (about D^2 / 2 for a gap of half-width D between two lines of
fixed cells).  Every value lies within [min, max] of the fixed values: the coarsest level starts from copies of its
fixed values, and every update is clamped to that range (the solution lies in it, so the clamp moves no fixed point).
A part of the domain that holds a single fixed value and stays closed off on every level of the pyramid holds that
value exactly; behind a wall thinner than the coarsest cell it holds it within tol * max(t).

Cost.  The rounds a level needs grow with the widest gap between fixed cells, counted in tiles: relaxation tile by tile
moves a smooth error across a tile border one cell of halo at a time, and the pyramid's start is off by a smooth error
of the order of one coarse cell times the gradient.  Voids of a few dozen cells take tens of rounds; a sparse river
network on a large raster takes thousands, and the default budget can run out at tol = 1e-5 (DESIGN.md 4.24 has the
measurements): raise tol (4096 rounds per level is the largest budget there is), or pass strict=False and take the
last iterate with the residual it reached.

Refused with ValueError before any library call: rasters that are not 2-D, shapes that differ, 2^31 cells or more, a tol
that is not finite and > 0, a max_rounds outside 1..4096, a negative max_cells.

Recipes.
    vd = harmonic.vdcn(dem, river)                       # into evaluation.calibration(vd, flood, under=True) and
                                                         # reaches.hydraulic_tables in HAND's place
    ridges = flowacc on the negated DEM, thresholded     # the channels of the terrain turned upside down
    valley_depth = np.where(dem > -100, harmonic.base_level(dem, ridges) - dem, -100)
    normalised_height = vd / (vd + valley_depth)         # 0 in the channel, 1 on the ridge
    dem = harmonic.fill_voids(dem)                       # before flowdir.d8_conditioned: a one-cell void is a barrier
                                                         # to D8 and a pit rim to the depression fill"""
import warnings

import numpy as np

from . import _args, _lib, regions
from ._lib import c_f32p, c_f64p, c_i8p, c_i64p, check, ptr
from .device import host_empty

INFO_WORDS = 40  # DT_HARMONIC_INFO_WORDS
ROUNDS_MAX = 4096


class Harmonic(tuple):
    """(field float64,) of interpolate, with `.field` and `.info`: {"levels": levels of the pyramid, "rounds": rounds of
    tile visits on the finest level, "rounds_all": on all levels, "rounds_per_level": a list, finest first,
    "tile_visits": visits of 64 x 64 tiles, "residual": the largest r of the field, "converged": residual <= tol,
    "unreached": free cells of the domain dropped for want of a fixed cell}"""

    def __new__(cls, field, info=None):
        self = tuple.__new__(cls, (field,))
        self.info = info
        return self

    field = property(lambda self: self[0])


def _tol(tol):
    return _args.positive(tol, "tol")


def _rounds(max_rounds):
    return _args.integer(max_rounds, "max_rounds", 1, ROUNDS_MAX)


def _solve(v, fx, dom, tol, max_rounds, strict=True):
    """the library call on checked arrays (v float32, fx and dom bool; dom holds fx) -> Harmonic; the cells of dom that
    no path joins to a fixed cell are dropped first.  When the budget runs out: RuntimeError, or with strict false a
    RuntimeWarning and the last iterate (info["converged"] is False)"""
    H, W = v.shape
    unreached = 0
    if v.size:
        reached = regions.connected(dom, fx, connectivity=4) != 0
        unreached = int(np.count_nonzero(dom & ~reached))
        dom = reached
    field = host_empty((H, W), np.float64)
    info = np.zeros(INFO_WORDS, np.int64)
    check(_lib.lib().dt_harmonic(ptr(v, c_f32p), ptr(np.ascontiguousarray(fx, np.int8), c_i8p),
                                 ptr(np.ascontiguousarray(dom, np.int8), c_i8p), H, W, tol, max_rounds,
                                 ptr(field, c_f64p), ptr(info, c_i64p)))
    levels = int(info[0])
    residual = float(info[4:5].view(np.float64)[0])
    out = {"levels": levels, "rounds": int(info[1]), "rounds_all": int(info[2]),
           "rounds_per_level": [int(x) for x in info[8:8 + levels]], "tile_visits": int(info[3]),
           "residual": residual, "converged": bool(info[5]) or v.size == 0, "unreached": unreached}
    if not out["converged"]:
        msg = ("harmonic: the residual is %.3g after %d rounds of tile visits on the finest level, above tol = %g: the "
               "budget max_rounds = %d ran out" % (residual, out["rounds"], tol, max_rounds))
        if strict:
            raise RuntimeError(msg)
        warnings.warn(msg + "; the field is the last iterate", RuntimeWarning, stacklevel=3)
    return Harmonic(field, out)


def interpolate(values, fixed, domain=None, tol=1e-5, max_rounds=4096, strict=True):
    """The harmonic function on `domain` that holds `values` on the cells with fixed == 1 -> Harmonic(field float64)
    with `.info`; NaN outside the domain and on cells without a value.  The module docstring holds the definition.
    `max_rounds` (1..4096) is the budget of rounds of tile visits per level of the pyramid; RuntimeError when it runs out
    on the finest level.  strict=False: a RuntimeWarning instead, and the last iterate with .info["converged"] False and
    .info["residual"] what it reached, so that the work is not thrown away."""
    v = _args.raster(values, "values", kinds="biuf")
    f = _args.raster(fixed, "fixed", shape=v.shape, other="values")
    d = None if domain is None else _args.raster(domain, "domain", shape=v.shape, other="values")
    t = _tol(tol)
    n = _rounds(max_rounds)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.ascontiguousarray(v, np.float32)
    one = np.asarray(f == 1)
    fx = one & np.isfinite(v)
    dom = fx | ~one if d is None else fx | (~one & np.asarray(d != 0))
    return _solve(v, fx, dom, t, n, bool(strict))


def select_voids(label, size, max_cells=None, edges=False):
    """Which cells fill_voids fills -> bool raster.  label, size: regions.label(nodata, 8, sizes=True) of the nodata mask
    (label = the smallest flat index of the cell's void, -100 on valid cells).  A void is filled when it does not touch
    the raster's border (edges=True: those too) and holds at most max_cells cells (None: any number).  Pure numpy."""
    lab = np.asarray(label)
    fill = lab >= 0
    if max_cells is not None:
        fill &= np.asarray(size) <= max_cells
    if not edges and lab.size:
        ring = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
        fill &= ~np.isin(lab, np.unique(ring[ring >= 0]))
    return fill


def fill_voids(dem, max_cells=None, edges=False, tol=1e-5):
    """The DEM in its own dtype with its voids filled by the harmonic interpolant of the valid cells around them; valid
    cells are bit-identical.  A void is an 8-connected region of nodata cells -- _lib.nodata_mask (dem <= -100) and,
    in a float DEM, NaN, the two forms holes arrive in; +-inf is neither valid nor a void and stays as it is.  A void is
    filled when it does not touch the raster's border (edges=True: those too) and holds at most max_cells cells.  The
    valid cells are fixed and only void cells are free, so the work grows with the voids, not with the raster.  The
    heights are interpolated as float32 values (an integer DEM gets the nearest integer); tol is interpolate's."""
    d = _args.raster(dem, "dem", kinds="iuf")
    cap = None if max_cells is None else _args.integer(max_cells, "max_cells", 0)
    t = _tol(tol)
    nod = _lib.nodata_mask(d, d.shape) != 0
    if d.dtype.kind == "f":
        nod |= np.isnan(d)
    out = np.array(d, copy=True)
    if not nod.any():
        return out
    lab, size = regions.label(nod, 8, sizes=True)
    fill = select_voids(lab, size, cap, bool(edges))
    if not fill.any():
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.ascontiguousarray(d, np.float32)
    fx = ~nod & np.isfinite(v)
    field = _solve(v, fx, fx | fill, t, ROUNDS_MAX).field
    got = fill & ~np.isnan(field)
    vals = field[got]
    out[got] = (np.rint(vals) if out.dtype.kind in "iu" else vals).astype(out.dtype)
    return out


def _base(dem, mask, tol, strict):
    """(the DEM as float32, base level as float64 with NaN where there is no value)"""
    d = _args.raster(dem, "dem", kinds="iuf")
    m = _args.raster(mask, "mask", shape=d.shape, other="dem")
    t = _tol(tol)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.ascontiguousarray(d, np.float32)
    valid = (_lib.nodata_mask(d, d.shape) == 0) & np.isfinite(v)
    return v, _solve(v, valid & np.asarray(m == 1), valid, t, ROUNDS_MAX, bool(strict)).field


def base_level(dem, mask, tol=1e-5, strict=True):
    """The surface that interpolates the DEM's heights on the cells with mask == 1 (a river network: SAGA's channel
    network base level; a ridge network: the level valley depth is measured from) over the valid cells -> float64, -100
    where there is no value (nodata, and valid cells that no path over valid cells joins to a mask cell).  The heights
    are taken as float32.  strict=False: when 4096 rounds per level do not reach tol, a RuntimeWarning and the last
    iterate instead of RuntimeError."""
    field = _base(dem, mask, tol, strict)[1]
    return np.where(np.isnan(field), -100.0, field)


def vdcn(dem, river, tol=1e-5, strict=True):
    """Vertical distance to channel network: the DEM minus base_level(dem, river) -> float64, -100 where there is no
    value.  Both terms are the float32 heights widened to float64, so a river cell holds exactly 0 whatever the DEM's
    dtype.  Not clipped at 0: a cell below the interpolated channel level is information -- which also means that a
    true distance of -100 or less (a cell 100 units below the channel level) cannot be told from the sentinel; on such
    terrain compare with base_level's -100 instead.  strict: as base_level's."""
    v, field = _base(dem, river, tol, strict)
    return np.where(np.isnan(field), -100.0, v.astype(np.float64) - field)
