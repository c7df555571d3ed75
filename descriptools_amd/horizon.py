"""What a cell sees along eight lines of sight (net-new): geomorphon landforms and their ternary patterns (Jasiewicz &
Stepinski 2013; GRASS r.geomorphon), positive and negative topographic openness (Yokoyama et al. 2002) and the sky-view
factor (Zaksek et al. 2011).  All of them derive from one quantity: from every cell, the highest and the lowest elevation
angle seen in each of eight compass directions, out to a search radius.

Validity.  A height is valid when it is finite and > -100, as everywhere in the package.

Directions.  d = 0..7 = N, NE, E, SE, S, SW, W, NW; the row / column steps (dy, dx) are (-1,0), (-1,1), (0,1), (1,1),
(1,0), (1,-1), (0,-1), (-1,-1).

Parameters.  radius L: an integer in [1, 64].  skip: an integer in [0, L - 1].  flat: degrees, finite, in [0, 90).

Samples.  For a valid centre (y, x) with height z0 the samples of direction d are the cells (y + k dy, x + k dx) for
k = skip + 1 .. L.  A sample counts only if it lies in the raster and is valid: invalid and outside cells are SKIPPED,
the line of sight goes on past them.

Arithmetic.  Everything is IEEE float64 on the float32 heights.

    step[0] = px                           cardinal directions
    step[1] = px * 1.4142135623730951      diagonal directions
    inv[c][k] = 1.0 / (float(k) * step[c])               tabulated once, on the host side of the C entry
    t = (float64(z_k) - float64(z0)) * inv[c][k]         the tangent of a sample

The tangent is a MULTIPLICATION by the tabulated reciprocal, not a division: that is the definition, not an
optimisation.  tmax_d is the maximum of t over the samples of direction d, tmin_d the minimum.

Cells with a value.  A cell HAS A VALUE iff its centre is valid and every one of the eight directions has at least one
sample.  Any other cell holds "no value" in every output: -100 in the float outputs, 0 in landform, 65535 in pattern.

Ternary digit of a direction.  T = math.tan(math.radians(flat)) is computed once here (flat_tangent) and passed down
as a double; the kernel has no trigonometry for it.  The digit follows r.geomorphon's comparison form -- the larger of
the two angles decides -- on tangents, because atan is monotone:

    1. if |tmax_d| > |tmin_d| and |tmax_d| > T the digit is +1 (the terrain rises above the cell that way)
    2. otherwise, if |tmin_d| > T and |tmax_d| <= |tmin_d| the digit is -1
    3. otherwise the digit is 0

A tie |tmax_d| == |tmin_d| > T falls to rule 2: -1, whatever the sign.  Every direction with a single sample is one
(radius 1, skip == radius - 1, the cell next to the rim), and so is, in exact arithmetic, every up-slope ray of an
exactly straight ramp, whose samples share one tangent: there the last bit of k * inv[c][k] decides between +1 and -1.
Real terrain has no such rays; synthetic planes and cones do.

Outputs (OUTPUTS), any subset, each once; only what is asked for is computed.

pattern   uint16    sum_d (digit_d + 1) 3^d, in 0..6560
landform  uint8     1 flat, 2 peak, 3 ridge, 4 shoulder, 5 spur, 6 slope, 7 hollow, 8 footslope, 9 valley, 10 pit
                    (LANDFORMS), read from LANDFORM_TABLE[m][p] with m the number of -1 digits and p of +1 digits:

                    m\\p   0   1   2   3   4   5   6   7   8
                    0     1   1   1   8   8   9   9   9  10
                    1     1   1   8   8   8   9   9   9
                    2     1   4   6   6   7   7   9
                    3     4   4   6   6   6   7
                    4     4   4   5   6   6
                    5     3   3   5   5
                    6     3   3   3
                    7     3   3
                    8     2

                    The table is this project's definition (after r.geomorphon's).  It is self-dual: swapping m and p
                    maps 2 <-> 10, 3 <-> 9, 4 <-> 8, 5 <-> 7 and leaves 1 and 6 fixed, so the landforms of c - dem are
                    the duals of the landforms of dem.
positive  float32   (sum_d (pi/2 - atan(tmax_d))) / 8.0, radians; the sum runs over d = 0..7 in order from its d = 0 term
negative  float32   (sum_d (pi/2 + atan(tmin_d))) / 8.0, radians, the same order
sky_view  float32   1.0 - (sum_d s_d) / 8.0, the same order, with s_d = tmax_d / sqrt(1.0 + tmax_d tmax_d) when
                    tmax_d > 0, else 0.0 (the sine of the horizon angle; no trigonometry)

pattern, landform and sky_view are built from + - * / sqrt and comparisons in this association and equal the numpy
reference of the test suite bit for bit; positive and negative hold eight atan each and are within one float32 spacing
of it.

Flood mapping.  A geomorphon class of hollow, footslope, valley or pit, and the openness of a cell, mark valley bottoms
and flood-prone cells without any flow direction, so they work on unconditioned DEMs, wide floodplains and coastal
plains (as proximity.euclidean_hand does).  They go into evaluation.calibration like any other descriptor:

    form = horizon.geomorphons(dem, px, radius=20)
    mask = np.isin(form, (7, 8, 9, 10)).astype(np.int8)       # a binary flood map as it stands
    neg = horizon.openness(dem, px, radius=20, kind="negative")
    evaluation.calibration(neg, observed, 'over')
    sky = horizon.sky_view(dem, px, radius=20)
    evaluation.calibration(sky, observed, 'under')

The sense.  With this definition negative openness is the mean angle from the nadir up to the lowest line of sight:
it is ABOVE pi/2 where the surroundings stand above the cell (valley floors, pits: tmin_d >= 0) and below pi/2 on
ridges and peaks, so the flood-prone cells are the HIGH ones: 'over'.  Positive openness and sky_view are low where the
horizon stands high -- a valley floor sees less sky than a plain or a ridge -- so the flood-prone cells are the LOW
ones: 'under'.  Cells without a value hold -100, the nodata value the evaluation functions leave out."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_u8p, c_u16p, check, ptr

OUTPUTS = ("landform", "pattern", "positive", "negative", "sky_view")
RADIUS_MAX = 64
LANDFORMS = {1: "flat", 2: "peak", 3: "ridge", 4: "shoulder", 5: "spur", 6: "slope", 7: "hollow", 8: "footslope",
             9: "valley", 10: "pit"}
# LANDFORM_TABLE[m][p]: m = number of -1 digits, p = number of +1 digits, m + p <= 8
LANDFORM_TABLE = ((1, 1, 1, 8, 8, 9, 9, 9, 10),
                  (1, 1, 8, 8, 8, 9, 9, 9),
                  (1, 4, 6, 6, 7, 7, 9),
                  (4, 4, 6, 6, 6, 7),
                  (4, 4, 5, 6, 6),
                  (3, 3, 5, 5),
                  (3, 3, 3),
                  (3, 3),
                  (2,))
_DTYPES = {"landform": (np.uint8, c_u8p), "pattern": (np.uint16, c_u16p), "positive": (np.float32, c_f32p),
           "negative": (np.float32, c_f32p), "sky_view": (np.float32, c_f32p)}
_KINDS = ("positive", "negative")


def flat_tangent(flat=1.0):
    """T = tan(flat degrees), the threshold the digits compare tangents with; ValueError unless flat is a number (not
    a bool), finite and in [0, 90)"""
    try:
        f = math.nan if isinstance(flat, (bool, np.bool_)) else float(flat)
    except (TypeError, ValueError):
        f = math.nan
    if not (math.isfinite(f) and 0.0 <= f < 90.0):
        raise ValueError("flat must be a finite number of degrees in [0, 90), not %r" % (flat,))
    return math.tan(math.radians(f))


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


def attributes(dem, px, outputs=("landform",), radius=10, skip=0, flat=1.0):
    """The line-of-sight attributes named in `outputs` (any of OUTPUTS, each once) of `dem` (float32-exact heights; a
    DEM that float32 cannot hold raises ValueError, as terrain.attributes does) -> dict {name: raster[H, W]} in the
    order asked for: landform uint8, pattern uint16, the others float32; the module docstring holds the definition.
    radius: an integer in [1, 64], the search radius in cells; skip: an integer in [0, radius - 1], the nearest cells
    left out of every line of sight; flat: the flatness threshold in degrees, in [0, 90).  Only what is asked for is
    computed; the cost per cell grows with 8 (radius - skip).  Bad arguments raise ValueError before any library
    call."""
    d = _args.raster(dem, "dem")
    p = _args.pixel_size(px)
    names = _outputs(outputs)
    r = _args.integer(radius, "radius", 1, RADIUS_MAX)
    s = _args.integer(skip, "skip", 0, r - 1)
    T = flat_tangent(flat)
    d = _lib.dem_f32(d)
    H, W = d.shape
    out = {n: np.empty((H, W), _DTYPES[n][0]) for n in names}
    check(_lib.lib().dt_horizon(ptr(d, c_f32p), H, W, p, r, s, T, *(ptr(out.get(n), _DTYPES[n][1]) for n in OUTPUTS)))
    return out


def geomorphons(dem, px, radius=10, skip=0, flat=1.0):
    """attributes' landform alone: uint8, 1..10 (LANDFORMS), 0 where there is no value"""
    return attributes(dem, px, ("landform",), radius, skip, flat)["landform"]


def openness(dem, px, radius=10, kind="positive", skip=0):
    """One openness of attributes, float32 radians, -100 where there is no value: kind is 'positive' (the mean zenith
    angle of the horizon: low in valleys, high on ridges) or 'negative' (the mean nadir angle: low in enclosed
    hollows and valley floors seen from below)"""
    if not isinstance(kind, str) or kind not in _KINDS:
        raise ValueError("kind must be one of %s, not %r" % (_KINDS, kind))
    return attributes(dem, px, (kind,), radius, skip)[kind]


def sky_view(dem, px, radius=10, skip=0):
    """attributes' sky_view alone: the sky-view factor in [0, 1], float32, -100 where there is no value"""
    return attributes(dem, px, ("sky_view",), radius, skip)["sky_view"]
