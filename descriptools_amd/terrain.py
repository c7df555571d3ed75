"""Local terrain attributes (net-new; Evans 1980, Wood 1996, the multiscale curvatures of current GIS tools): gradient,
aspect, profile / plan / tangential / mean curvature, the Laplacian and hillshade of the quadratic surface fitted by
least squares over the (2 radius + 1)^2 window of every cell.  radius 1 is Evans' 3 x 3 scheme; on 1-2 m LiDAR rasters
a 3 x 3 curvature is mostly noise, which is what the radius is for.

Window and validity.  A height is valid when it is finite and > -100, as everywhere in the package.  With
n = 2 radius + 1 a cell HAS A VALUE iff all n^2 heights of the window centred on it lie in the raster and are valid.
Every other cell -- nodata, a NaN or +-inf centre, any cell within `radius` of the rim or of an invalid cell -- holds
-100 in every output: -100 means "no value".  A curvature of -100 m^-1 or below does not occur on a physical DEM;
gradient == -100 is the mask when one is wanted.

All arithmetic is IEEE float64.  Sums run left to right from their first term; the offsets i (columns, east positive)
and j (rows, south positive) run over -radius .. radius in ascending order; an integer factor is converted to float64
and multiplied before each addition.  With z the float32 height as float64:

column pass    C0(y, x) = sum_j z(y + j, x)    C1 = sum_j (-j) z    C2 = sum_j (j j) z
row pass       M00 = sum_i C0(y, x + i)    M10 = sum_i i C0    M20 = sum_i (i i) C0
               M01 = sum_i C1              M11 = sum_i i C1    M02 = sum_i C2

Derivatives of the fitted quadratic at the centre; x is east, y is north, h = px, r the radius:
S2 = r (r + 1) (2 r + 1) / 3, S4 = r (r + 1) (2 r + 1) (3 r^2 + 3 r - 1) / 15, D = n S4 - S2^2 (integers, exact in
float64 for r <= 32); den1 = float(n S2) h, den2 = float(S2^2) (h h), den3 = float(n D) (h h);

    p = M10 / den1    q = M01 / den1    s = M11 / den2
    r = 2.0 ((n M20 - S2 M00) / den3)    t = 2.0 ((n M02 - S2 M00) / den3)

(z_x, z_y, z_xy, z_xx, z_yy).  For radius 1: p = (z3 + z6 + z9 - z1 - z4 - z7) / (6 h), r = (z1 + z3 + z4 + z6 + z7 + z9
- 2 (z2 + z5 + z8)) / (3 h^2) with Evans' numbering.

Outputs, each float32(value), with w = p p + q q, g1 = 1.0 + w, pq2 = 2.0 (p q):

gradient      sqrt(w): rise over run (degrees are np.degrees(np.arctan(gradient)) on the host)
aspect        the compass bearing of the downslope direction, degrees clockwise from north:
              a = atan2(-p, -q) * 57.29577951308232, plus 360.0 when a < 0; rounded to float32, and 0 when that is
              >= 360; -1 when w == 0 (flat)
profile       -(((p p) r + pq2 s) + (q q) t) / (w (g1 sqrt(g1)))     along the slope line
plan          -(((q q) r - pq2 s) + (p p) t) / (w sqrt(w))           contour curvature
tangential    plan's numerator over w sqrt(g1)
              profile, plan and tangential are 0 when w == 0
mean          -(((1.0 + q q) r - pq2 s) + (1.0 + p p) t) / (2.0 (g1 sqrt(g1)))
laplacian     r + t
hillshade     ((sz - p sx) - q sy) / sqrt(g1), 0 when that is not > 0: in [0, 1];
              (sx, sy, sz) = (sin az cos alt, cos az cos alt, sin alt), computed here once with `math` and passed down
              as three doubles, so the kernel has no trigonometry

Sign.  Positive curvature is CONVEX (ridges, domes, divergent noses), negative is CONCAVE (valleys, convergent hollows):
a spherical cap of radius R has profile = tangential = mean = +1 / R.  For a flood descriptor that means `under`
(evaluation.calibration(..., under=True)): the low, convergent cells are the flood-prone ones.

Every output but aspect is built from + - * / sqrt in this association and equals the numpy reference of the test
suite bit for bit; aspect has one atan2 and is within one float32 spacing of it."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, check, ptr

OUTPUTS = ("gradient", "aspect", "profile", "plan", "tangential", "mean", "laplacian", "hillshade")
CURVATURES = OUTPUTS[2:7]
RADIUS_MAX = 32


def _finite(v, what):
    try:
        f = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not math.isfinite(f):
        raise ValueError("%s must be a finite number, not %r" % (what, v))
    return f


def sun_vector(azimuth=315.0, altitude=45.0):
    """The unit vector to the sun (east, north, up) of a compass azimuth and an altitude above the horizon, both in
    degrees; ValueError unless azimuth is finite and altitude finite and in (0, 90]"""
    az = _finite(azimuth, "azimuth")
    alt = _finite(altitude, "altitude")
    if not 0.0 < alt <= 90.0:
        raise ValueError("altitude must lie in (0, 90], not %r" % (altitude,))
    az, alt = math.radians(az), math.radians(alt)
    return math.sin(az) * math.cos(alt), math.cos(az) * math.cos(alt), math.sin(alt)


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


def attributes(dem, px, outputs=("gradient", "aspect"), radius=1, azimuth=315.0, altitude=45.0):
    """The terrain attributes named in `outputs` (any of OUTPUTS, each once) of `dem` (float32-exact heights; a DEM
    that float32 cannot hold raises ValueError, as dinf.flow_direction does) -> dict {name: float32[H, W]} in the order
    asked for; the module docstring holds the definition.  radius: an integer in [1, 32], the window is
    (2 radius + 1)^2 cells; azimuth (finite) and altitude (in (0, 90]) place hillshade's sun, in degrees.  Only what
    is asked for is computed; the cost per cell grows with radius.  Bad arguments raise ValueError before any library
    call."""
    d = _args.raster(dem, "dem")
    p = _args.pixel_size(px)
    names = _outputs(outputs)
    r = _args.integer(radius, "radius", 1, RADIUS_MAX)
    sx, sy, sz = sun_vector(azimuth, altitude)
    d = _lib.dem_f32(d)
    H, W = d.shape
    out = {n: np.empty((H, W), np.float32) for n in names}
    check(_lib.lib().dt_terrain(ptr(d, c_f32p), H, W, p, r, sx, sy, sz, *(ptr(out.get(n), c_f32p) for n in OUTPUTS)))
    return out


def gradient(dem, px, radius=1):
    """attributes' gradient alone: rise over run, float32, -100 where there is no value"""
    return attributes(dem, px, ("gradient",), radius)["gradient"]


def aspect(dem, px, radius=1):
    """attributes' aspect alone: degrees clockwise from north of the downslope direction, -1 on flat cells"""
    return attributes(dem, px, ("aspect",), radius)["aspect"]


def curvature(dem, px, kind="profile", radius=1):
    """One curvature of attributes: kind is 'profile', 'plan', 'tangential', 'mean' or 'laplacian'; positive is convex"""
    if not isinstance(kind, str) or kind not in CURVATURES:
        raise ValueError("kind must be one of %s, not %r" % (CURVATURES, kind))
    return attributes(dem, px, (kind,), radius)[kind]


def hillshade(dem, px, azimuth=315.0, altitude=45.0, radius=1):
    """attributes' hillshade alone: the cosine of the angle between the surface normal and the sun, in [0, 1]"""
    return attributes(dem, px, ("hillshade",), radius, azimuth, altitude)["hillshade"]
