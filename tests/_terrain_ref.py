"""The numpy reference of descriptools_amd.terrain: with that module's docstring, the definition.  Vectorised over
shifted slices, one addition per offset, so every sum has the kernel's association: from its first term, in ascending
offset, the integer factor converted to float64 and multiplied before the addition.  A height that is not valid, or
lies outside the raster, enters the sums as NaN: M00 is NaN exactly where the window is not complete."""
import math

import numpy as np

OUTPUTS = ("gradient", "aspect", "profile", "plan", "tangential", "mean", "laplacian", "hillshade")
NODATA = np.float32(-100)


def valid(dem):
    d = np.asarray(dem)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > -100)


def constants(radius, px):
    """(n, S2, den1, den2, den3): n and S2 as float64"""
    r = int(radius)
    n = 2 * r + 1
    S2 = r * (r + 1) * (2 * r + 1) // 3
    S4 = r * (r + 1) * (2 * r + 1) * (3 * r * r + 3 * r - 1) // 15
    D = n * S4 - S2 * S2
    h = float(px)
    return float(n), float(S2), float(n * S2) * h, float(S2 * S2) * (h * h), float(n * D) * (h * h)


def moments(dem, radius):
    """(M00, M10, M20, M01, M11, M02) of every cell, float64[H, W]; NaN where the window is not complete.  The
    heights are taken as they are, as float64: the package accepts a DEM only when float32 holds every height, and on
    such a DEM this is the definition; on other heights (the sphere of the host tests) it is the same fit unrounded."""
    d = np.asarray(dem)
    H, W = d.shape
    r = int(radius)
    zp = np.full((H + 2 * r, W + 2 * r), np.nan)
    zp[r:r + H, r:r + W] = np.where(valid(d), d.astype(np.float64), np.nan)
    with np.errstate(invalid="ignore"):
        C0 = C1 = C2 = None
        for j in range(-r, r + 1):
            z = zp[r + j:r + j + H, :]
            t1, t2 = float(-j) * z, float(j * j) * z
            if C0 is None:
                C0, C1, C2 = z.copy(), t1, t2
            else:
                C0, C1, C2 = C0 + z, C1 + t1, C2 + t2
        M = None
        for i in range(-r, r + 1):
            c0, c1, c2 = (C[:, r + i:r + i + W] for C in (C0, C1, C2))
            t = [c0, float(i) * c0, float(i * i) * c0, c1, float(i) * c1, c2]
            M = [x.copy() for x in t] if M is None else [m + x for m, x in zip(M, t)]
    return tuple(M)


def derivatives(dem, px, radius):
    """(p, q, r, s, t, has_value) of the fitted quadratic at every cell: z_x, z_y, z_xx, z_xy, z_yy with x east and
    y north; NaN where has_value is False"""
    M00, M10, M20, M01, M11, M02 = moments(dem, radius)
    n, S2, den1, den2, den3 = constants(radius, px)
    with np.errstate(invalid="ignore"):
        p = M10 / den1
        q = M01 / den1
        s = M11 / den2
        r = 2.0 * ((n * M20 - S2 * M00) / den3)
        t = 2.0 * ((n * M02 - S2 * M00) / den3)
    return p, q, r, s, t, ~np.isnan(M00)


def sun_vector(azimuth, altitude):
    az, alt = math.radians(float(azimuth)), math.radians(float(altitude))
    return math.sin(az) * math.cos(alt), math.cos(az) * math.cos(alt), math.sin(alt)


def attributes(dem, px, outputs=OUTPUTS, radius=1, azimuth=315.0, altitude=45.0):
    """-> dict {name: float32[H, W]} of the outputs asked for, -100 where a cell has no value"""
    p, q, r, s, t, has = derivatives(dem, px, radius)
    sx, sy, sz = sun_vector(azimuth, altitude)
    with np.errstate(all="ignore"):
        pp, qq = p * p, q * q
        w = pp + qq
        g1 = 1.0 + w
        pq2 = 2.0 * (p * q)
        sg1 = np.sqrt(g1)
        flat = w == 0
        v = {}
        v["gradient"] = np.sqrt(w).astype(np.float32)
        a = np.arctan2(-p, -q) * 57.29577951308232
        a = np.where(a < 0, a + 360.0, a)
        a32 = a.astype(np.float32)
        a32[a32 >= np.float32(360)] = 0
        a32[flat] = -1
        v["aspect"] = a32
        v["profile"] = np.where(flat, 0.0, -((pp * r + pq2 * s) + qq * t) / (w * (g1 * sg1))).astype(np.float32)
        num = -((qq * r - pq2 * s) + pp * t)
        v["plan"] = np.where(flat, 0.0, num / (w * np.sqrt(w))).astype(np.float32)
        v["tangential"] = np.where(flat, 0.0, num / (w * sg1)).astype(np.float32)
        v["mean"] = (-(((1.0 + qq) * r - pq2 * s) + (1.0 + pp) * t) / (2.0 * (g1 * sg1))).astype(np.float32)
        v["laplacian"] = (r + t).astype(np.float32)
        hs = ((sz - p * sx) - q * sy) / sg1
        v["hillshade"] = np.where(hs > 0, hs, 0.0).astype(np.float32)
    return {k: np.where(has, v[k], NODATA) for k in outputs}


# ---- surfaces whose derivatives are known (the host and the GPU tests share them) ------------------------------------
def plane(H, W, a, b, c=1000):
    """z = c + a x + b y on integers: x = column (east), y = -row (north)"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (c + a * xx - b * yy).astype(np.float32)


def paraboloid(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((xx - W // 2) ** 2 + (yy - H // 2) ** 2).astype(np.float32)


def sphere_cap(H, W, R_, px):
    """the upper cap of a sphere of radius R_ centred under the raster's middle"""
    yy, xx = np.mgrid[0:H, 0:W]
    x, y = (xx - (W - 1) / 2) * px, (yy - (H - 1) / 2) * px
    return np.sqrt(R_ * R_ - x * x - y * y)
