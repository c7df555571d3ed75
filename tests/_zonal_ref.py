"""Pure-numpy reference of descriptools_amd.zonal, independent of the kernels: np.unique for compact, np.bincount and
np.add.at with Python-int (object) sums for the tables, np.histogram per zone, fancy indexing for paint, and the float
stage of statistics written once more, here.

Shared by tests/test_zonal_host.py (which checks it against explicit per-zone Python loops on small rasters) and
tests/test_gpu_zonal.py (which holds the GPU to it entry for entry, bit for bit).  The product never imports it."""
import math

import numpy as np

QMAX = 2 ** 31 - 1
NONE = -100


def compact(labels, limit=None):
    """(zones int32, labels_of int64)"""
    lb = np.asarray(labels).astype(np.int64)
    lim = max(lb.size, 1) if limit is None else limit
    valid = (lb >= 0) & (lb < lim)
    labels_of = np.unique(lb[valid]).astype(np.int64)
    zones = np.full(lb.shape, NONE, np.int32)
    zones[valid] = np.searchsorted(labels_of, lb[valid]).astype(np.int32)
    return zones, labels_of


def values_of(values):
    """values as the library reads them: float32 as it is, everything else as float64"""
    v = np.asarray(values)
    return v if v.dtype == np.float32 else v.astype(np.float64)


def taking_part(zones, values, n_zones, nodata=-100.0):
    """the mask of the cells that have a zone and a finite value other than nodata"""
    z = np.asarray(zones).astype(np.int64)
    v = values_of(values).astype(np.float64)
    m = (z >= 0) & (z < n_zones) & np.isfinite(v)
    if nodata is not None:
        m &= v != np.float64(nodata)
    return m


def quantise(v, origin, s):
    """int64(rint((float64(v) - origin) 2^s)) of finite values (object array where it leaves int64)"""
    with np.errstate(over="ignore"):
        return np.rint(np.ldexp(np.asarray(v, np.float64) - np.float64(origin), s))


def default_scale(zones, values, n_zones, nodata=-100.0, frac_bits=None, origin=None):
    """(origin, frac_bits): floor of the smallest participating value, the largest s <= 16 within the contract"""
    m = taking_part(zones, values, n_zones, nodata)
    v = values_of(values)[m].astype(np.float64)
    o = origin if origin is not None else (float(math.floor(v.min())) if v.size else 0.0)
    if frac_bits is not None:
        return float(o), frac_bits
    for s in range(16, -1, -1):
        if not v.size or max(abs(int(quantise(v.min(), o, s))), abs(int(quantise(v.max(), o, s)))) <= QMAX:
            return float(o), s
    raise AssertionError("the values fit no frac_bits")


def sum_squares(z, q, n_zones, limbs=None):
    """the sum of q^2 per zone as Python ints (object array).  Up to 2^17 cells: np.add.at on Python ints.  Beyond
    (or with limbs=True): q^2 < 2^62 in three limbs of 21 bits, each summed by np.bincount with float64 weights (exact:
    a limb sum stays below 2^31 * 2^21 = 2^52), put together as Python ints per zone."""
    if limbs is None:
        limbs = q.size > 1 << 17
    if not limbs:
        qo = q.astype(object)
        s2 = np.zeros(n_zones, object)
        np.add.at(s2, z, qo * qo)
        return s2
    q2 = (q * q).astype(np.uint64)
    parts = [np.bincount(z, weights=((q2 >> np.uint64(21 * k)) & np.uint64(0x1FFFFF)).astype(np.float64),
                         minlength=n_zones) for k in range(3)]
    s2 = np.zeros(n_zones, object)
    for k in range(3):
        s2 += np.array([int(x) << (21 * k) for x in parts[k]], object)
    return s2


def tables(zones, values, n_zones, origin, s, nodata=-100.0):
    """dict of count, s1 (int64), s2 (object: Python ints, the whole sum of q^2), s2_lo, s2_hi (uint64), vmin, vmax
    (the dtype the library reads the values in; NaN on empty zones), and out (the number of cells whose q is outside
    the contract, which the library leaves out and reports)"""
    v = values_of(values)
    m = taking_part(zones, v, n_zones, nodata)
    z = np.asarray(zones).astype(np.int64)[m]
    x = v[m]
    x = np.where(x == 0, x.dtype.type(0), x)  # -0.0 counts as +0.0
    qf = quantise(x, origin, s)
    ok = np.abs(qf) <= QMAX
    out = int((~ok).sum())
    z, x, q = z[ok], x[ok], qf[ok].astype(np.int64)
    count = np.bincount(z, minlength=n_zones).astype(np.int64)
    s1 = np.zeros(n_zones, np.int64)
    np.add.at(s1, z, q)
    s2 = sum_squares(z, q, n_zones)
    q2 = (q * q).astype(np.uint64)  # |q| < 2^31: q^2 < 2^62
    lo = np.zeros(n_zones, np.uint64)
    hi = np.zeros(n_zones, np.uint64)
    np.add.at(lo, z, q2 & np.uint64(0xFFFFFFFF))
    np.add.at(hi, z, q2 >> np.uint64(32))
    assert all(int(h) * 2 ** 32 + int(l) == int(t) for h, l, t in zip(hi, lo, s2))
    vmin = np.full(n_zones, np.nan, x.dtype)
    vmax = np.full(n_zones, np.nan, x.dtype)
    if z.size:
        order = np.lexsort((x, z))
        zs, xs = z[order], x[order]
        first = np.flatnonzero(np.r_[True, zs[1:] != zs[:-1]])
        last = np.r_[first[1:] - 1, zs.size - 1]
        vmin[zs[first]] = xs[first]
        vmax[zs[first]] = xs[last]
    return {"count": count, "s1": s1, "s2": s2, "s2_lo": lo, "s2_hi": hi, "vmin": vmin, "vmax": vmax, "out": out}


def statistics(t, origin, s):
    """the float stage, in the association of the module docstring of descriptools_amd.zonal: dict of every output"""
    u = 2.0 ** -s
    with np.errstate(divide="ignore", invalid="ignore"):
        nf = t["count"].astype(np.float64)
        s1f = t["s1"].astype(np.float64)
        m = s1f / nf
        s2f = np.ldexp(t["s2_hi"].astype(np.float64), 32) + t["s2_lo"].astype(np.float64)
        var = s2f / nf - m * m
        var = np.where(var < 0, 0.0, var)
        return {"count": t["count"].copy(), "sum": nf * origin + s1f * u, "mean": origin + m * u,
                "std": np.sqrt(var) * u, "min": t["vmin"].astype(np.float64), "max": t["vmax"].astype(np.float64),
                "range": t["vmax"].astype(np.float64) - t["vmin"].astype(np.float64)}


def histogram(zones, values, n_zones, edges, nodata=-100.0):
    """int64[n_zones, K]: np.histogram of every zone's participating values"""
    e = np.asarray(edges, np.float64)
    v = values_of(values).astype(np.float64)
    m = taking_part(zones, v, n_zones, nodata)
    z = np.asarray(zones).astype(np.int64)
    out = np.zeros((n_zones, e.size - 1), np.int64)
    for k in np.unique(z[m]):
        out[k] = np.histogram(v[m & (z == k)], bins=e)[0]
    return out


def crosstab(a, b, n_a, n_b):
    """int64[n_a, n_b]: the cells with a == i and b == j, both in range"""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    m = (a >= 0) & (a < n_a) & (b >= 0) & (b < n_b)
    return np.bincount(a[m] * n_b + b[m], minlength=n_a * n_b).reshape(n_a, n_b).astype(np.int64)


def paint(table, zones, fill):
    tb = np.asarray(table)
    z = np.asarray(zones).astype(np.int64)
    ok = (z >= 0) & (z < tb.size)
    out = np.full(z.shape, fill, tb.dtype)
    out[ok] = tb[z[ok]]
    return out


def quantile_loop(hist_row, edges, p):
    """one zone's quantile by a plain loop over its bins"""
    total = int(hist_row.sum())
    if total == 0:
        return math.nan
    t = p * total
    cum = 0
    for k, c in enumerate(hist_row):
        c = int(c)
        if c and (cum + c >= t):
            return float(edges[k] + (t - cum) / c * (edges[k + 1] - edges[k]))
        cum += c
    return float(edges[-1])


def ids_per_tile(zones, n_zones, tile=64):
    """the largest number of distinct in-range zone ids that one tile x tile tile of the raster holds"""
    z = np.asarray(zones)
    worst = 0
    for y in range(0, z.shape[0], tile):
        for x in range(0, z.shape[1], tile):
            t = z[y:y + tile, x:x + tile]
            worst = max(worst, np.unique(t[(t >= 0) & (t < n_zones)]).size)
    return worst
