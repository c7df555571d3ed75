"""The numpy reference of descriptools_amd.horizon: with that module's docstring, the definition.  8 x radius steps over
shifted slices of a NaN-padded float64 copy of the heights; np.fmax / np.fmin return the operand that is not NaN, so a
sample that is not valid, or lies outside the raster, drops out of the extremes and a direction without a sample is a
maximum that is still NaN.  The tangent is a multiplication by the tabulated reciprocal, as in the kernel."""
import math

import numpy as np

OUTPUTS = ("landform", "pattern", "positive", "negative", "sky_view")
NODATA = np.float32(-100)
STEPS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))  # N NE E SE S SW W NW: (dy, dx)
HALF_PI = 1.5707963267948966
# TABLE[m][p]: m = the number of -1 digits, p = of +1 digits; 0 where m + p > 8
TABLE = np.array([[1, 1, 1, 8, 8, 9, 9, 9, 10],
                  [1, 1, 8, 8, 8, 9, 9, 9, 0],
                  [1, 4, 6, 6, 7, 7, 9, 0, 0],
                  [4, 4, 6, 6, 6, 7, 0, 0, 0],
                  [4, 4, 5, 6, 6, 0, 0, 0, 0],
                  [3, 3, 5, 5, 0, 0, 0, 0, 0],
                  [3, 3, 3, 0, 0, 0, 0, 0, 0],
                  [3, 3, 0, 0, 0, 0, 0, 0, 0],
                  [2, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
DUAL = np.array([0, 1, 10, 9, 8, 7, 6, 5, 4, 3, 2], np.uint8)  # the landform of the surface turned upside down


def valid(dem):
    d = np.asarray(dem)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > -100)


def flat_tangent(flat):
    return math.tan(math.radians(float(flat)))


def reciprocals(px, radius):
    """inv[c][k] for k = 0 .. radius (entry 0 unused); c = 0 cardinal, 1 diagonal"""
    step = (float(px), float(px) * 1.4142135623730951)
    return [[math.nan] + [1.0 / (float(k) * step[c]) for k in range(1, int(radius) + 1)] for c in range(2)]


def extremes(dem, px, radius, skip=0):
    """(tmax, tmin): float64[8, H, W], NaN where a direction has no sample or the centre is not valid"""
    d = np.asarray(dem)
    H, W = d.shape
    L = int(radius)
    inv = reciprocals(px, L)
    zp = np.full((H + 2 * L, W + 2 * L), np.nan)
    zp[L:L + H, L:L + W] = np.where(valid(d), d.astype(np.float64), np.nan)
    z0 = zp[L:L + H, L:L + W]
    tmax = np.full((8, H, W), np.nan)
    tmin = np.full((8, H, W), np.nan)
    with np.errstate(invalid="ignore"):
        for dd, (dy, dx) in enumerate(STEPS):
            for k in range(int(skip) + 1, L + 1):
                zk = zp[L + k * dy:L + k * dy + H, L + k * dx:L + k * dx + W]
                t = (zk - z0) * inv[dd & 1][k]
                tmax[dd] = np.fmax(tmax[dd], t)
                tmin[dd] = np.fmin(tmin[dd], t)
    return tmax, tmin


def digits(tmax, tmin, T):
    """the ternary digit of every direction, int8[8, H, W] (0 where tmax is NaN)"""
    with np.errstate(invalid="ignore"):
        a, b = np.abs(tmax), np.abs(tmin)
        plus = (a > b) & (a > T)
        minus = ~plus & (b > T) & (a <= b)
    return plus.astype(np.int8) - minus.astype(np.int8)


def decode(pattern):
    """the eight digits of a pattern raster, int8[8, H, W]"""
    p = np.asarray(pattern).astype(np.int64)
    return np.stack([(p // 3 ** d) % 3 - 1 for d in range(8)]).astype(np.int8)


def attributes(dem, px, T, outputs=OUTPUTS, radius=10, skip=0):
    """-> dict {name: raster[H, W]} of the outputs asked for; T is the flatness tangent, a double"""
    tmax, tmin = extremes(dem, px, radius, skip)
    has = ~np.isnan(tmax).any(axis=0)
    dg = digits(tmax, tmin, float(T)).astype(np.int64)
    v = {}
    v["pattern"] = np.where(has, sum((dg[d] + 1) * 3 ** d for d in range(8)), 65535).astype(np.uint16)
    m, p = (dg == -1).sum(axis=0), (dg == 1).sum(axis=0)
    v["landform"] = np.where(has, TABLE[m, p], 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        pos = neg = sky = None
        for d in range(8):
            tp = HALF_PI - np.arctan(tmax[d])
            tn = HALF_PI + np.arctan(tmin[d])
            s = np.where(tmax[d] > 0, tmax[d] / np.sqrt(1.0 + tmax[d] * tmax[d]), 0.0)
            pos, neg, sky = (tp, tn, s) if d == 0 else (pos + tp, neg + tn, sky + s)
        v["positive"] = np.where(has, (pos / 8.0).astype(np.float32), NODATA)
        v["negative"] = np.where(has, (neg / 8.0).astype(np.float32), NODATA)
        v["sky_view"] = np.where(has, (1.0 - sky / 8.0).astype(np.float32), NODATA)
    return {k: np.ascontiguousarray(v[k]) for k in outputs}


# ---- surfaces whose landforms are known (the host and the GPU tests share them) -----------------------------------
# On an exactly straight flank every sample of an up-slope ray has the same tangent, tmax == tmin > T, and the digit
# rule sends that tie to -1 (rule 2 holds with |tmax| <= |tmin|): whether an ideal ramp reads +1 or -1 up-slope is then
# a matter of the last bit of a rounding.  `curl` lets the flanks steepen slightly with the distance s (s + curl s^2
# for s), far above the float32 rounding of the heights, so that the tangents of a ray grow with k.
def _flank(s, curl):
    return s + curl * s * s


def plane_east(H, W, rise=1.0, c=100.0, curl=0.0):
    """z = c + rise * column: rising to the east"""
    _, xx = np.mgrid[0:H, 0:W]
    return (c + rise * _flank(xx.astype(np.float64), curl)).astype(np.float32)


def cone(n, rise=1.0, c=100.0, curl=0.0):
    """a cone with its apex at the middle of an n x n raster (n odd): z = c - rise * distance in cells"""
    yy, xx = np.mgrid[0:n, 0:n]
    return (c - rise * _flank(np.hypot(yy - n // 2, xx - n // 2), curl)).astype(np.float32)


def valley_ns(H, W, rise=1.0, c=100.0, curl=0.0):
    """a V-valley whose axis runs north-south down the middle column: z = c + rise * |column - W // 2|"""
    _, xx = np.mgrid[0:H, 0:W]
    return (c + rise * _flank(np.abs(xx - W // 2).astype(np.float64), curl)).astype(np.float32)
