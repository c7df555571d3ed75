"""The numpy reference of descriptools_amd.focal, and a brute-force check of its integers.  With focal.py's module
docstring this is the specification: uint64 cumsum both ways (numpy wraps silently), four-corner differences modulo
2^64, and the float stage written line for line.  brute() sums explicit window loops in Python integers; it is slow and
used on rasters of at most 40 x 50 cells and on the wrap case."""
import math

import numpy as np

OUTPUTS = ("count", "mean", "std", "tpi", "dev")


def qmax(radius):
    """the largest integer q with (2 radius + 1)^2 q^2 < 2^63"""
    m = (2 * radius + 1) ** 2
    q = math.isqrt((2 ** 63 - 1) // m)
    assert m * q * q < 2 ** 63 <= m * (q + 1) ** 2
    return q


def valid(dem):
    d = np.asarray(dem, np.float32)
    return np.isfinite(d) & (d > np.float32(-100))


def quantise(dem, origin, frac_bits):
    """(valid, q int64): q = int64(rint((float64(z) - origin) * 2^s)) on valid cells, 0 elsewhere"""
    d = np.asarray(dem, np.float32)
    ok = valid(d)
    z = np.where(ok, d, np.float32(0)).astype(np.float64)
    q = np.rint((z - np.float64(origin)) * np.float64(2.0 ** frac_bits)).astype(np.int64)
    return ok, np.where(ok, q, 0)


def planes(ok, q):
    """the inclusive 2-D prefix sums of [valid], q and q^2, uint64 with wrap-around"""
    u = q.astype(np.uint64)
    cum = lambda a: np.cumsum(np.cumsum(a, axis=0, dtype=np.uint64), axis=1, dtype=np.uint64)
    return cum(ok.astype(np.uint64)), cum(u), cum(u * u)


def window_sum(P, radius):
    """the sum over the clipped (2 radius + 1)^2 window of every cell: the four-corner difference modulo 2^64"""
    H, W = P.shape
    y, x = np.arange(H), np.arange(W)
    ya, yb = np.maximum(y - radius, 0) - 1, np.minimum(y + radius, H - 1)
    xa, xb = np.maximum(x - radius, 0) - 1, np.minimum(x + radius, W - 1)
    Z = np.zeros((H + 1, W + 1), np.uint64)  # row 0 and column 0: the empty prefix
    Z[1:, 1:] = P
    at = lambda yy, xx: Z[(yy + 1)[:, None], (xx + 1)[None, :]]
    return at(yb, xb) - at(ya, xb) - at(yb, xa) + at(ya, xa)


def nab(dem, radius, origin, frac_bits):
    """(valid, q, n, A, B), n, A, B as int64 rasters (whatever they hold on cells without a value)"""
    ok, q = quantise(dem, origin, frac_bits)
    Pn, P1, P2 = planes(ok, q)
    n, S1, S2 = window_sum(Pn, radius), window_sum(P1, radius), window_sum(P2, radius)
    qc = q.astype(np.uint64)
    A = S1 - n * qc
    B = S2 - np.uint64(2) * qc * S1 + n * qc * qc
    return ok, q, n.astype(np.int64), A.view(np.int64), B.view(np.int64)


def _moments(n, A, B):
    with np.errstate(divide="ignore", invalid="ignore"):
        nf = n.astype(np.float64)
        a = A.astype(np.float64) / nf
        b = B.astype(np.float64) / nf
        var = b - a * a
        var = np.where(var < 0.0, 0.0, var)
        sd = np.sqrt(var)
    return a, sd


def _dev64(a, sd):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sd == 0.0, 0.0, (-a) / sd)


def statistics(dem, radius, origin, frac_bits):
    """{name: raster} of all five outputs"""
    ok, q, n, A, B = nab(dem, radius, origin, frac_bits)
    a, sd = _moments(n, A, B)
    u = np.float64(2.0 ** -frac_bits)
    with np.errstate(invalid="ignore"):
        mean = (np.float64(origin) + (q.astype(np.float64) + a) * u).astype(np.float32)
        std = (sd * u).astype(np.float32)
        tpi = ((-a) * u).astype(np.float32)
        dev = _dev64(a, sd).astype(np.float32)
    return {"count": np.where(ok, n, 0).astype(np.int32),
            "mean": np.where(ok, mean, np.float32(-100)),
            "std": np.where(ok, std, np.float32(-100)),
            "tpi": np.where(ok, tpi, np.float32("nan")),
            "dev": np.where(ok, dev, np.float32("nan"))}


def dev_max(dem, radii, origin, frac_bits):
    """(dev float32, scale uint16): the d_k of largest magnitude, a tie keeps the smaller radius"""
    best = at = None
    for r in radii:
        ok, _, n, A, B = nab(dem, r, origin, frac_bits)
        d = _dev64(*_moments(n, A, B))
        if best is None:
            best, at = d, np.full(d.shape, r, np.uint16)
        else:
            with np.errstate(invalid="ignore"):
                take = np.abs(d) > np.abs(best)
            best, at = np.where(take, d, best), np.where(take, np.uint16(r), at)
    with np.errstate(invalid="ignore"):
        dev = best.astype(np.float32)
    return np.where(ok, dev, np.float32("nan")), np.where(ok, at, np.uint16(0)).astype(np.uint16)


def brute(dem, radius, origin, frac_bits):
    """[(y, x, n, A, B)] of every valid cell, in Python integers over explicit window loops"""
    ok, q = quantise(dem, origin, frac_bits)
    H, W = ok.shape
    ql = [[int(v) for v in row] for row in q]
    okl = ok.tolist()
    out = []
    for y in range(H):
        for x in range(W):
            if not okl[y][x]:
                continue
            qc, n, A, B = ql[y][x], 0, 0, 0
            for yy in range(max(y - radius, 0), min(y + radius, H - 1) + 1):
                for xx in range(max(x - radius, 0), min(x + radius, W - 1) + 1):
                    if okl[yy][xx]:
                        t = ql[yy][xx] - qc
                        n, A, B = n + 1, A + t, B + t * t
            out.append((y, x, n, A, B))
    return out


def default_origin(dem):
    ok = valid(dem)
    return float(math.floor(np.asarray(dem, np.float32)[ok].min())) if ok.any() else 0.0


WRAP = dict(radius=5, origin=0.0, frac_bits=16)


def wrap_case():
    """150 x 150 heights uniform in [0, 1024) m: at origin 0 and frac_bits 16 the sum of q^2 over the raster exceeds
    2^64 (the table wraps) while a window of radius 5 holds at most 121 * 2^52 = 0.06 * 2^63"""
    return np.random.default_rng(2).uniform(0.0, 1024.0, (150, 150)).astype(np.float32)


def terrain(H, W, seed, holes=True, lo=100.0, hi=400.0):
    """a test raster: smooth relief plus noise; with `holes` ~8 % nodata in blobs and a NaN, +inf, -inf and -150 cell"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    z = 0.5 * (lo + hi) + 0.3 * (hi - lo) * np.sin(x / 17.0) * np.cos(y / 23.0) + rng.uniform(-1, 1, (H, W)) * 0.2 * (hi - lo)
    d = np.clip(z, lo, hi).astype(np.float32)
    if holes:
        n_blobs = max(1, (H * W) // 400)
        for _ in range(n_blobs):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 5)
            d[max(cy - r, 0):cy + r, max(cx - r, 0):cx + r] = -100 if rng.random() < 0.7 else -9999
        flat = d.reshape(-1)
        if flat.size >= 8:
            pick = rng.choice(flat.size, 4, replace=False)
            flat[pick[0]], flat[pick[1]], flat[pick[2]], flat[pick[3]] = np.nan, np.inf, -np.inf, -150
    return d
