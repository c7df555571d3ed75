"""Focal statistics at any radius (net-new): the count, mean and standard deviation of the heights in the
(2 radius + 1)^2 window of every cell, and from them the relative-position descriptors -- the topographic position index
TPI (Weiss 2001), the deviation from mean elevation DEV (De Reu et al. 2013) and the multi-scale maximum elevation
deviation DEVmax with the scale at which it occurs (Lindsay et al. 2015).  The cost per cell does not depend on the
radius: the window sums are four-corner differences of summed-area tables.

Validity.  A height is valid iff it is finite and > -100, as everywhere in the package.

Quantisation.  With `origin` (a finite float64) and s = frac_bits the quantised height of a valid cell is
q = int64(rint((float64(z) - origin) * 2^s)), rint to even.  Invalid cells contribute nothing.

Window.  The window of radius R around (y, x) is the (2 R + 1)^2 square clipped to the raster; invalid cells inside it
are skipped, not a stop.  A cell HAS A VALUE iff its own height is valid (a complete-window rule would blank the whole
raster at R = 1000).  For a cell with quantised height q_c, over the valid cells i of its window, three integers are
exact:  n, the count;  A = sum (q_i - q_c);  B = sum (q_i - q_c)^2.

Table planes.  The inclusive two-dimensional prefix sums of [valid], q and q^2, the latter two uint64 with wrap-around.
A window sum is the usual four-corner difference, taken modulo 2^64;
    A = S1 - n q_c        B = S2 - 2 q_c S1 + n q_c^2        both modulo 2^64, then read as signed 64-bit integers.
The tables wrap freely; every window sum that itself fits 63 bits still comes out exactly, so the result does not
depend on how the scan is associated, scheduled or tiled.

Contract that makes this exact.  0 <= q <= qmax(R_max), where qmax(R) is the largest integer with
(2 R + 1)^2 qmax^2 < 2^63 (integer arithmetic) and R_max the largest radius of the call.  A valid height outside the
contract raises DT_STATUS_BAD_HEIGHT in the library, which fails the call; the functions here see it from the smallest
and largest valid height before any library call and raise ValueError.

Float stage, all IEEE float64, in exactly this association (int64 -> float64 rounds to nearest even):
    nf = float64(n)    a = float64(A) / nf    b = float64(B) / nf
    var = b - a a, set to 0 when negative    sd = sqrt(var)    u = 2^-s

Outputs                                                        no value
    count  int32    n                                          0
    mean   float32  origin + (float64(q_c) + a) u              -100
    std    float32  sd u  (population)                         -100
    tpi    float32  (-a) u, i.e. z - mean                      NaN
    dev    float32  (-a) / sd, 0.0 when sd == 0                NaN
tpi and dev take NaN and not -100 because every real number is a legitimate value of them; the evaluation layer skips
NaN cells.  A strongly negative DEV is a valley floor: evaluation.calibration(..., under=True).

DEVmax, over a strictly increasing table of 1 to 32 radii: per cell the float64 d_k = (-a_k) / sd_k (0 when sd_k == 0)
of every radius; the one of largest |d_k| is kept, a tie keeps the smaller radius.  dev is that d_k as float32 (NaN
for no value), scale the radius as uint16 (0 for no value).

Every output equals the numpy reference of the test suite bit for bit."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_i32p, c_u16p, check, ptr

OUTPUTS = ("count", "mean", "std", "tpi", "dev")
RADIUS_MAX = 4096
RADII_MAX = 32
FRAC_BITS_MAX = 24
# 2^-16 m is finer than any DEM: the ceiling of the default frac_bits
_DEFAULT_FRAC_BITS_MAX = 16


def qmax(radius):
    """The largest integer q with (2 radius + 1)^2 q^2 < 2^63: the bound of a quantised height at that radius"""
    r = _args.integer(radius, "radius", 1, RADIUS_MAX)
    return math.isqrt((2 ** 63 - 1) // (2 * r + 1) ** 2)


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


def _radii(radii):
    if isinstance(radii, (str, bytes)) or not hasattr(radii, "__iter__"):
        raise ValueError("radii must be a sequence of integers, not %r" % (radii,))
    rs = tuple(radii)
    if not 1 <= len(rs) <= RADII_MAX:
        raise ValueError("radii must hold 1 to %d radii, not %d" % (RADII_MAX, len(rs)))
    rs = tuple(_args.integer(r, "a radius", 1, RADIUS_MAX) for r in rs)
    if any(b <= a for a, b in zip(rs, rs[1:])):
        raise ValueError("radii must be strictly increasing, not %r" % (rs,))
    return rs


def _range(d):
    """(smallest, largest) valid height of a float32 raster as floats, None without a valid cell"""
    valid = np.isfinite(d) & (d > np.float32(-100))
    if not valid.any():
        return None
    v = d[valid]
    return float(v.min()), float(v.max())


def _quantised(z, origin, s):
    return int(np.rint(np.ldexp(np.float64(z) - np.float64(origin), s)))


def _default_origin(rng):
    return 0.0 if rng is None else float(math.floor(rng[0]))


def _default_frac_bits(rng, origin, radius_max):
    if rng is None:
        return _DEFAULT_FRAC_BITS_MAX
    bound = qmax(radius_max)
    for s in range(_DEFAULT_FRAC_BITS_MAX, -1, -1):
        if _quantised(rng[1], origin, s) <= bound:
            return s
    raise ValueError("heights from %r to %r do not fit radius %d even at frac_bits=0: rint(max - origin) must be <= %d "
                     "(origin %r); use a smaller radius" % (rng[0], rng[1], radius_max, bound, origin))


def _origin(origin):
    if origin is None:
        return None
    try:
        f = math.nan if isinstance(origin, (bool, np.bool_)) else float(origin)
    except (TypeError, ValueError):
        f = math.nan
    if not math.isfinite(f):
        raise ValueError("origin must be a finite number, not %r" % (origin,))
    return f


def default_frac_bits(dem, radius_max, origin=None):
    """The default fixed-point scale of `dem` at the largest radius `radius_max`: the largest s in [0, 16] with
    rint((zmax - origin) * 2^s) <= qmax(radius_max), origin = floor(the smallest valid height) unless one is given;
    16 without a valid cell.  ValueError when s = 0 does not fit, naming the height range and the radius."""
    d = _lib.dem_f32(_args.raster(dem, "dem"))
    r = _args.integer(radius_max, "radius_max", 1, RADIUS_MAX)
    o = _origin(origin)
    rng = _range(d)
    return _default_frac_bits(rng, _default_origin(rng) if o is None else o, r)


def _scale(d, radius_max, frac_bits, origin):
    """(origin, frac_bits) of a call: the defaults where None, ValueError where they break the contract"""
    o = _origin(origin)
    if frac_bits is not None:
        frac_bits = _args.integer(frac_bits, "frac_bits", 0, FRAC_BITS_MAX)
    rng = _range(d)
    if o is None:
        o = _default_origin(rng)
    if frac_bits is None:
        frac_bits = _default_frac_bits(rng, o, radius_max)
    if rng is not None:
        lo, hi, bound = _quantised(rng[0], o, frac_bits), _quantised(rng[1], o, frac_bits), qmax(radius_max)
        if lo < 0:
            raise ValueError("origin=%r lies above the smallest valid height %r: quantised heights must be >= 0"
                             % (o, rng[0]))
        if hi > bound:
            raise ValueError("frac_bits=%d is too fine for heights up to %r above origin=%r at radius %d: "
                             "rint((z - origin) * 2^frac_bits) reaches %d, the bound is %d"
                             % (frac_bits, rng[1], o, radius_max, hi, bound))
    return o, frac_bits


def _call(d, o, s, radii, out):
    H, W = d.shape
    rs = np.asarray(radii, np.int32)
    check(_lib.lib().dt_focal(ptr(d, c_f32p), H, W, o, s, ptr(rs, c_i32p), len(radii), ptr(out.get("count"), c_i32p),
                              *(ptr(out.get(n), c_f32p) for n in OUTPUTS[1:]), ptr(out.get("scale"), c_u16p)))


def statistics(dem, radius, outputs=("tpi",), frac_bits=None, origin=None):
    """The focal statistics named in `outputs` (any of OUTPUTS, each once) of `dem` (float32-exact heights; a DEM that
    float32 cannot hold raises ValueError, as terrain.attributes does) over the window of `radius` (an integer in
    [1, 4096]) -> dict {name: raster[H, W]} in the order asked for; count is int32, the others float32.  The module
    docstring holds the definition.  origin defaults to floor(the smallest valid height), frac_bits to
    default_frac_bits; an explicit one that breaks the contract raises ValueError.  Only what is asked for is computed;
    the cost per cell does not depend on the radius.  Bad arguments raise ValueError before any library call."""
    d = _args.raster(dem, "dem")
    r = _args.integer(radius, "radius", 1, RADIUS_MAX)
    names = _outputs(outputs)
    d = _lib.dem_f32(d)
    o, s = _scale(d, r, frac_bits, origin)
    out = {n: np.empty(d.shape, np.int32 if n == "count" else np.float32) for n in names}
    _call(d, o, s, (r,), out)
    return out


def mean(dem, radius, frac_bits=None, origin=None):
    """statistics' mean alone: the mean height of the window, float32, -100 where there is no value"""
    return statistics(dem, radius, ("mean",), frac_bits, origin)["mean"]


def std(dem, radius, frac_bits=None, origin=None):
    """statistics' std alone: the population standard deviation of the window's heights, -100 where there is no value"""
    return statistics(dem, radius, ("std",), frac_bits, origin)["std"]


def tpi(dem, radius, frac_bits=None, origin=None):
    """statistics' tpi alone: the height minus the window's mean height, NaN where there is no value"""
    return statistics(dem, radius, ("tpi",), frac_bits, origin)["tpi"]


def dev(dem, radius, frac_bits=None, origin=None):
    """statistics' dev alone: tpi over the window's standard deviation, 0 on a level window, NaN without a value"""
    return statistics(dem, radius, ("dev",), frac_bits, origin)["dev"]


def dev_max(dem, radii, frac_bits=None, origin=None):
    """The multi-scale maximum elevation deviation of `dem` over `radii` (a strictly increasing sequence of 1 to 32
    integers in [1, 4096]) -> (dev float32[H, W], scale uint16[H, W]): per cell the DEV of largest magnitude and the
    radius it occurs at (a tie keeps the smaller radius); NaN and 0 where there is no value.  frac_bits and origin as
    in statistics, for the largest radius."""
    d = _args.raster(dem, "dem")
    rs = _radii(radii)
    d = _lib.dem_f32(d)
    o, s = _scale(d, rs[-1], frac_bits, origin)
    out = {"dev": np.empty(d.shape, np.float32), "scale": np.empty(d.shape, np.uint16)}
    _call(d, o, s, rs, out)
    return out["dev"], out["scale"]
