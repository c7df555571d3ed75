"""Zonal statistics (net-new), on the GPU: what a value raster does inside every zone of a label raster -- the count,
sum, mean, standard deviation, minimum, maximum and range per zone, per-zone histograms (and from them quantiles: the
median, the hypsometric curve), the cross-tabulation of two zone rasters -- with the two steps around it: making sparse
labels dense (compact) and painting a per-zone table back onto the raster (paint).  The label rasters of
watershed.basins / watersheds and regions.label (flat indices, sparse in [0, H W)) go through compact first; those of
reaches.catchments, horizon.geomorphons and evaluation.binary_map are dense already.

Definitions (the kernels in csrc/dt_zonal.hip, the C header and the tests hold to them).  Rasters are H x W, row-major,
N = H * W < 2^31.

* compact.  A label l is valid when 0 <= l < limit (limit defaults to N, what flat-index labels need; 1 <= limit <=
  2^31 - 1).  labels_of (int64[n_zones]) = the distinct valid labels in ascending order (np.unique of the valid
  labels).  zones (int32) = the rank of the cell's label in labels_of, -100 where the label is not valid.
* Zones.  zones is int32 (int64 is accepted when it fits).  A cell has a zone when 0 <= z < n_zones; negative values
  have no zone; a value >= n_zones is an error (ValueError here, from the raster's maximum; DT_STATUS_ZONE_RANGE on the
  device tier, where the cell is left out).
* Participation.  values is float32 or float64, each read as it is; any other real or integer dtype is converted to
  float64.  A cell takes part when it has a zone, its value is finite, and its value (as float64) is not equal to
  nodata; nodata=None means no such value.  -0.0 counts as +0.0.
* Quantisation.  With s = frac_bits in [0, 24] and a finite origin, q = int64(rint((float64(v) - origin) * 2^s)), rint
  to even; q may be negative.  Contract: |q| <= 2^31 - 1.  A value outside it raises DT_STATUS_BAD_HEIGHT in the
  library and counts as not taking part, which fails a host-tier call; the functions here see it from the range of the
  participating values before any library call and raise ValueError.  Defaults: origin = floor(the smallest
  participating value), frac_bits = the largest s <= 16 that keeps the contract.
* Tables, per zone over its participating cells, all exact:
      count   n                          int64
      s1      sum q                      int64 (|sum q| < 2^62)
      s2_lo   sum (q^2 mod 2^32)         uint64
      s2_hi   sum (q^2 div 2^32)         uint64      sum q^2 = s2_hi 2^32 + s2_lo; each part stays below 2^63
      vmin    the smallest value         the dtype of values; NaN on a zone without a participating cell
      vmax    the largest value          likewise
  vmin and vmax are the values themselves, not their quantised forms.  Only the accumulators named in `want` (count,
  s1, s2, min, max) are computed and allocated.
* Float stage of statistics, numpy float64 on the tables, in exactly this association:
      nf  = float64(n)      m = float64(s1) / nf      S2f = ldexp(float64(s2_hi), 32) + float64(s2_lo)
      var = S2f / nf - m m, set to 0 when negative         u = 2^-s
  Outputs                                                       empty zone
      count  int64    n                                          0
      sum    float64  nf origin + float64(s1) u                  0.0
      mean   float64  origin + m u                               NaN
      std    float64  sqrt(var) u  (population)                  NaN
      min    float64  float64(vmin)                              NaN
      max    float64  float64(vmax)                              NaN
      range  float64  float64(vmax) - float64(vmin)              NaN
  std carries the cancellation of S2f / nf - m^2: its absolute error is about |m| u 2^-26, m the zone's mean in
  quantised units above the origin, which is why the origin defaults to the floor of the smallest value and not to 0.
* histogram.  edges is float64[K + 1], finite and strictly increasing, 1 <= K <= 1024.  A participating cell counts in
  bin k when edges[k] <= v < edges[k + 1]; the last bin also takes v == edges[K] (np.histogram's rule); comparisons in
  float64 on the exact value.  The result is int64[n_zones, K]; n_zones * K * 8 bytes may not exceed 2 GiB.
* crosstab.  counts[i, j] (int64[n_a, n_b], 1 <= n_b <= 1024, the same 2 GiB cap) = the number of cells with a = i and
  b = j; cells where either raster is negative count nowhere; a >= n_a or b >= n_b is an error as for zones.
* paint.  out[c] = table[zones[c]] where 0 <= zones[c] < len(table), else fill; table is float32, float64, int32 or
  int64 and the output has its dtype.

Every table, zone raster and painted raster equals the numpy reference of the test suite bit for bit, and so do the
derived floats.  Bad arguments raise ValueError before any library call.  Users of a resident chain call the
dt_dev_zonal_* entries on their device rasters and statistics_from_tables on the tables."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from . import _args, _lib, reaches
from ._lib import c_f64p, c_i32p, c_i64p, check, ptr

Compact = namedtuple("Compact", ["zones", "labels_of"])
ZoneTables = namedtuple("ZoneTables", ["count", "s1", "s2_lo", "s2_hi", "vmin", "vmax", "origin", "frac_bits"])

ACCUMULATORS = ("count", "s1", "s2", "min", "max")
OUTPUTS = ("count", "sum", "mean", "std", "min", "max", "range")
FRAC_BITS_MAX = 24
QMAX = 2 ** 31 - 1
MAX_BINS = 1024
MAX_TABLE_BYTES = 2 ** 31
_DEFAULT_FRAC_BITS_MAX = 16
_ZONES_CAP = 1 << 20  # labels asked for in the first call; a raster with more zones takes a second, lighter call
_NEEDS = {"count": ("count",), "sum": ("count", "s1"), "mean": ("count", "s1"), "std": ("count", "s1", "s2"),
          "min": ("min",), "max": ("max",), "range": ("min", "max")}
_PAINT_DTYPES = (np.float32, np.float64, np.int32, np.int64)


def _names(names, allowed, what):
    if isinstance(names, str) or not hasattr(names, "__iter__"):
        raise ValueError("%s must be a sequence of names from %s, not %r" % (what, allowed, names))
    names = tuple(names)
    if not names:
        raise ValueError("%s is empty; name at least one of %s" % (what, allowed))
    for n in names:
        if not isinstance(n, str) or n not in allowed:
            raise ValueError("%s: %r is not one of %s" % (what, n, allowed))
    if len(set(names)) != len(names):
        raise ValueError("%s names an entry twice: %r" % (what, names))
    return names


def _number(v, what):
    try:
        f = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not math.isfinite(f):
        raise ValueError("%s must be a finite number, not %r" % (what, v))
    return f


def _values(values, shape):
    """(array, element size): float32 and float64 as they are, anything else real or integer as float64"""
    v = _args.raster(values, "values", shape, "the zone raster", kinds="biuf")
    if v.dtype == np.float32:
        return np.ascontiguousarray(v), 4
    return np.ascontiguousarray(v, np.float64), 8


def _zones(zones, n_zones, what="zones", count="n_zones", shape=None, other=None, hi=2 ** 31 - 1, lo=0):
    z = reaches._ids32(zones, what, shape, other)
    nz = _args.integer(n_zones, count, lo, hi)
    if z.size and int(z.max()) >= nz:
        raise ValueError("%s holds the id %d, %s is %d" % (what, int(z.max()), count, nz))
    return z, nz


def _nodata(nodata):
    return None if nodata is None else _number(nodata, "nodata")


def _range(z, v, nodata):
    """(smallest, largest) participating value as floats, None without one"""
    m = (z >= 0) & np.isfinite(v)
    if nodata is not None:
        m &= v != np.float64(nodata)
    if not m.any():
        return None
    p = v[m]
    return float(p.min()), float(p.max())


def _quantised(v, origin, s):
    """|rint((v - origin) 2^s)| as an int, 2^63 when it is not finite"""
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(np.ldexp(np.float64(v) - np.float64(origin), s))
    return abs(int(q)) if np.isfinite(q) else 2 ** 63


def _scale(rng, frac_bits, origin):
    """(origin, frac_bits) of a call: the defaults where None, ValueError where they break the contract"""
    o = None if origin is None else _number(origin, "origin")
    if frac_bits is not None:
        frac_bits = _args.integer(frac_bits, "frac_bits", 0, FRAC_BITS_MAX)
    if o is None:
        o = 0.0 if rng is None else float(math.floor(rng[0]))
    if rng is None:
        return o, _DEFAULT_FRAC_BITS_MAX if frac_bits is None else frac_bits
    reach = lambda s: max(_quantised(rng[0], o, s), _quantised(rng[1], o, s))
    if frac_bits is None:
        for s in range(_DEFAULT_FRAC_BITS_MAX, -1, -1):
            if reach(s) <= QMAX:
                return o, s
        raise ValueError("values from %r to %r do not fit even at frac_bits=0: |rint(v - origin)| must be <= %d "
                         "(origin %r)" % (rng[0], rng[1], QMAX, o))
    if reach(frac_bits) > QMAX:
        raise ValueError("frac_bits=%d is too fine for values from %r to %r around origin=%r: "
                         "|rint((v - origin) * 2^frac_bits)| reaches %d, the bound is %d"
                         % (frac_bits, rng[0], rng[1], o, reach(frac_bits), QMAX))
    return o, frac_bits


def _labels(labels):
    lb = reaches._ids(labels, "labels")
    if lb.dtype == np.int32:
        return np.ascontiguousarray(lb), 4
    return np.ascontiguousarray(lb, np.int64), 8


def compact(labels, limit=None):
    """Compact(zones, labels_of) of an int32 or int64 label raster: labels_of (int64[n_zones]) the distinct labels in
    [0, limit) in ascending order, zones (int32 raster) the rank of each cell's label among them, -100 where the label
    is outside [0, limit).  limit defaults to the number of cells (flat-index labels: watershed.basins,
    regions.label); see the module docstring."""
    lb, nbytes = _labels(labels)
    H, W = lb.shape
    n = H * W
    lim = max(n, 1) if limit is None else _args.integer(limit, "limit", 1, 2 ** 31 - 1)
    zones = np.empty((H, W), np.int32)
    cap = min(lim, n, _ZONES_CAP)
    labels_of = np.empty(cap, np.int64)
    nz = C.c_int64(0)
    L = _lib.lib()
    check(L.dt_zonal_compact(lb.ctypes.data_as(C.c_void_p), nbytes, H, W, lim, ptr(zones, c_i32p),
                             ptr(labels_of, c_i64p) if cap else None, cap, C.byref(nz)))
    Z = int(nz.value)
    if Z > cap:  # the labels alone, at their size
        labels_of = np.empty(Z, np.int64)
        check(L.dt_zonal_compact(lb.ctypes.data_as(C.c_void_p), nbytes, H, W, lim, None, ptr(labels_of, c_i64p), Z,
                                 C.byref(nz)))
    return Compact(zones, labels_of[:Z].copy() if Z < labels_of.size else labels_of)


def tables(zones, values, n_zones, frac_bits=None, origin=None, nodata=-100.0, want=ACCUMULATORS):
    """ZoneTables(count, s1, s2_lo, s2_hi, vmin, vmax, origin, frac_bits): the exact per-zone accumulators of `values`
    over `zones` (each [n_zones]; None where `want`, a sequence of names from ACCUMULATORS, leaves it out) with the
    origin and frac_bits they were taken at; see the module docstring."""
    z, nz = _zones(zones, n_zones)
    v, vb = _values(values, z.shape)
    nd = _nodata(nodata)
    names = _names(want, ACCUMULATORS, "want")
    o, s = _scale(_range(z, v, nd), frac_bits, origin)
    H, W = z.shape
    new = lambda name, dtype: np.zeros(nz, dtype) if name in names else None
    count, s1 = new("count", np.int64), new("s1", np.int64)
    lo, hi = new("s2", np.uint64), new("s2", np.uint64)
    vmin, vmax = new("min", v.dtype), new("max", v.dtype)
    vpp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    check(_lib.lib().dt_zonal_tables(ptr(z, c_i32p), vpp(v), vb, H, W, nz, o, s, int(nd is not None),
                                     0.0 if nd is None else nd, ptr(count, c_i64p), ptr(s1, c_i64p), vpp(lo), vpp(hi),
                                     vpp(vmin), vpp(vmax)))
    return ZoneTables(count, s1, lo, hi, vmin, vmax, o, s)


def statistics_from_tables(t, outputs=("count", "mean")):
    """The outputs named in `outputs` (any of OUTPUTS, each once) from a ZoneTables that holds what they need -> dict
    {name: array[n_zones]} in the order asked for: host arithmetic on n_zones numbers, in the association of the
    module docstring."""
    names = _names(outputs, OUTPUTS, "outputs")
    have = {"count": t.count, "s1": t.s1, "s2": t.s2_lo, "min": t.vmin, "max": t.vmax}
    for n in names:
        for a in _NEEDS[n]:
            if have[a] is None:
                raise ValueError("output %r needs the accumulator %r, which the tables do not hold" % (n, a))
    out = {}
    u = 2.0 ** -t.frac_bits
    with np.errstate(divide="ignore", invalid="ignore"):
        if t.count is not None:
            nf = t.count.astype(np.float64)
        if t.s1 is not None and t.count is not None:
            s1f = t.s1.astype(np.float64)
            m = s1f / nf
        for n in names:
            if n == "count":
                out[n] = t.count.copy()
            elif n == "sum":
                out[n] = nf * t.origin + s1f * u
            elif n == "mean":
                out[n] = t.origin + m * u
            elif n == "std":
                s2f = np.ldexp(t.s2_hi.astype(np.float64), 32) + t.s2_lo.astype(np.float64)
                var = s2f / nf - m * m
                out[n] = np.sqrt(np.where(var < 0, 0.0, var)) * u
            elif n == "min":
                out[n] = t.vmin.astype(np.float64)
            elif n == "max":
                out[n] = t.vmax.astype(np.float64)
            else:
                out[n] = t.vmax.astype(np.float64) - t.vmin.astype(np.float64)
    return out


def statistics(zones, values, n_zones, outputs=("count", "mean"), frac_bits=None, origin=None, nodata=-100.0):
    """The zonal statistics named in `outputs` (any of OUTPUTS, each once) of `values` over `zones` -> dict
    {name: array[n_zones]} in the order asked for; count is int64, the others float64, NaN (sum: 0.0) on a zone
    without a participating cell.  Only the accumulators the outputs need are computed; see the module docstring."""
    names = _names(outputs, OUTPUTS, "outputs")
    want = tuple(a for a in ACCUMULATORS if any(a in _NEEDS[n] for n in names))
    return statistics_from_tables(tables(zones, values, n_zones, frac_bits, origin, nodata, want), names)


def _edges(edges):
    try:
        e = np.ascontiguousarray(edges, np.float64)
    except (TypeError, ValueError):
        raise ValueError("edges must be a 1-D array of numbers") from None
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError("edges must be a 1-D array of 2 to %d values, not of shape %s" % (MAX_BINS + 1, e.shape))
    if not np.isfinite(e).all():
        raise ValueError("edges must be finite")
    if not (np.diff(e) > 0).all():
        raise ValueError("edges must be strictly increasing")
    return e


def _table_cap(nz, K):
    if nz * K * 8 > MAX_TABLE_BYTES:
        raise ValueError("a table of %d zones x %d columns takes %d bytes; the cap is 2 GiB" % (nz, K, nz * K * 8))


def histogram(zones, values, n_zones, edges, nodata=-100.0):
    """The histogram of `values` in every zone over the bins of `edges` (float64[K + 1], np.histogram's rule) ->
    int64[n_zones, K]; see the module docstring."""
    z, nz = _zones(zones, n_zones)
    v, vb = _values(values, z.shape)
    e = _edges(edges)
    nd = _nodata(nodata)
    K = e.size - 1
    _table_cap(nz, K)
    H, W = z.shape
    counts = np.zeros((nz, K), np.int64)
    check(_lib.lib().dt_zonal_counts(ptr(z, c_i32p), v.ctypes.data_as(C.c_void_p), vb, H, W, nz, ptr(e, c_f64p), K,
                                     int(nd is not None), 0.0 if nd is None else nd, ptr(counts, c_i64p)))
    return counts


def crosstab(a, b, n_a, n_b):
    """The cross-tabulation of two zone rasters -> int64[n_a, n_b]: counts[i, j] = the cells with a == i and b == j
    (1 <= n_b <= 1024); see the module docstring."""
    za, na = _zones(a, n_a, "a", "n_a")
    zb, nb = _zones(b, n_b, "b", "n_b", za.shape, "the raster a", MAX_BINS, 1)
    _table_cap(na, nb)
    H, W = za.shape
    counts = np.zeros((na, nb), np.int64)
    check(_lib.lib().dt_zonal_counts(ptr(za, c_i32p), zb.ctypes.data_as(C.c_void_p), 0, H, W, na, None, nb, 0, 0.0,
                                     ptr(counts, c_i64p)))
    return counts


def quantiles(hist, edges, q):
    """The quantiles q (a number or a 1-D sequence in [0, 1]) of every zone of a histogram (int64[n_zones, K] over
    float64[K + 1] edges), linearly interpolated inside the bin that holds them -> float64[n_zones] for a number,
    float64[n_zones, len(q)] for a sequence; NaN on a zone without a count.  q = 0.5 is the median; the quantiles
    1 - a of a DEM per basin are its hypsometric curve.  numpy on the host."""
    h = np.asarray(hist)
    e = _edges(edges)
    if h.ndim != 2 or h.shape[1] != e.size - 1 or h.dtype.kind not in "iu" or (h.size and int(h.min()) < 0):
        raise ValueError("hist must be a non-negative integer array of shape (n_zones, %d)" % (e.size - 1))
    try:
        qq = np.asarray(q, np.float64)
    except (TypeError, ValueError):
        raise ValueError("q must be a number or a 1-D sequence of numbers in [0, 1]") from None
    if qq.ndim > 1 or not ((qq >= 0) & (qq <= 1)).all():
        raise ValueError("q must be a number or a 1-D sequence of numbers in [0, 1]")
    Z, K = h.shape
    cum = np.cumsum(h.astype(np.float64), axis=1)
    total = cum[:, -1] if K else np.zeros(Z)
    out = np.full((Z, qq.size), np.nan)
    rows = np.arange(Z)
    for i, p in enumerate(qq.reshape(-1)):
        t = p * total
        # the first bin whose cumulative count reaches t; for t == 0 the first bin with a count
        k = np.where(t > 0, (cum < t[:, None]).sum(axis=1), (cum <= 0).sum(axis=1))
        k = np.minimum(k, K - 1)
        before = cum[rows, k] - h[rows, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, i] = e[k] + (t - before) / h[rows, k] * (e[k + 1] - e[k])
        out[total == 0, i] = np.nan
    return out[:, 0] if qq.ndim == 0 else out


def paint(table, zones, fill):
    """The raster out[c] = table[zones[c]] where 0 <= zones[c] < len(table), else `fill`, in the dtype of `table`
    (float32, float64, int32 or int64, 1-D): a per-zone result back on its zones, e.g.
    hand / paint(statistics(...)["range"], zones, nan)."""
    tb = np.asarray(table)
    if tb.ndim != 1 or tb.dtype.type not in _PAINT_DTYPES or tb.size >= 2 ** 31:
        raise ValueError("table must be a 1-D array of float32, float64, int32 or int64 with fewer than 2^31 entries, "
                         "not %s of shape %s" % (tb.dtype, tb.shape))
    tb = np.ascontiguousarray(tb)
    z = reaches._ids32(zones, "zones")
    if tb.dtype.kind == "f":
        try:
            f = np.array([math.nan if isinstance(fill, (bool, np.bool_, str)) else float(fill)], tb.dtype)
        except (TypeError, ValueError):
            f = None
        if f is None or (f[0] != f[0] and not (isinstance(fill, (float, np.floating)) and fill != fill)):
            raise ValueError("fill must be a number, not %r" % (fill,))
    else:
        info = np.iinfo(tb.dtype)
        f = np.array([_args.integer(fill, "fill", int(info.min), int(info.max))], tb.dtype)
    H, W = z.shape
    out = np.empty((H, W), tb.dtype)
    check(_lib.lib().dt_zonal_paint(tb.ctypes.data_as(C.c_void_p), tb.dtype.itemsize, tb.size, ptr(z, c_i32p), H, W,
                                    f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out
