"""Flow accumulation (net-new): number of upstream cells EXCLUDING self, the
convention of the bundled 12_fac.tif; int64 like the `fac` the reference's callers pass.

accumulate_weighted sums a weight raster down the same D8 tree instead of counting cells (runoff or rainfall depth,
per-cell area, a load), in int64 fixed point so that the result is exact and deterministic."""
import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i64p, c_u8p, check, nodata_mask, ptr


def accumulate(fdr, dem=None):
    fdr = _args.raster(fdr, "fdr", cap=False, dtype=np.uint8)  # the size limit is the library's (dt_check_hw)
    d = nodata_mask(dem, fdr.shape)  # the DEM is only a nodata mask here
    H, W = fdr.shape
    acc = np.empty((H, W), np.int64)
    check(_lib.lib().dt_flowacc_u8(ptr(fdr, c_u8p), ptr(d, c_f32p), H, W, ptr(acc, c_i64p)))
    return acc


def _weights_f64(weights, shape=None):
    """weights -> C-contiguous float64, ValueError for anything outside the contract: real or integer dtype, finite,
    >= 0, integers <= 2^53 (exact in float64)"""
    a = np.asarray(weights)
    if shape is not None and a.shape != shape:
        raise ValueError("weights have shape %s, the direction raster %s" % (a.shape, shape))
    if a.dtype.kind not in "biuf":
        raise ValueError("weights must be of a real or integer dtype, not %s" % a.dtype)
    if a.dtype.kind in "iu" and a.size:
        if a.dtype.kind == "i" and int(a.min()) < 0:
            raise ValueError("weights must be >= 0 (the smallest is %d)" % int(a.min()))
        if int(a.max()) > 2 ** 53:
            raise ValueError("integer weights must be <= 2^53 (float64 holds them exactly); the largest is %d"
                             % int(a.max()))
    d = np.ascontiguousarray(a, dtype=np.float64)
    if a.dtype.kind == "f" and d.size:
        if not np.isfinite(d).all():
            raise ValueError("weights must be finite (NaN or infinity at flat index %d)"
                             % int(np.argmin(np.isfinite(d).reshape(-1))))
        if not (d >= 0).all():
            raise ValueError("weights must be >= 0 (the smallest is %r)" % float(d.min()))
    return d


def _countdown_accumulate(entry, raster, raster_type, shape, weights, frac_bits, fourth):
    """What dinf.accumulate and mfd.accumulate do once their direction raster is validated: the weights, frac_bits,
    the library's `entry` (by name) on `raster` -> (acc, w or None, s, info), info = {rounds, queue_high, queued, and
    the count the caller calls `fourth`}"""
    H, W = shape
    n = H * W
    w = None if weights is None else _weights_f64(weights, (H, W))
    wmax = 1.0 if w is None else (float(w.max()) if n else 0.0)
    s = _args.frac_bits(n, wmax, frac_bits, " for these weights: N * rint(max(weights) * 2^frac_bits)",
                        "the default is")
    acc = np.empty((H, W), np.float64)
    info = np.zeros(4, np.int64)
    check(getattr(_lib.lib(), entry)(ptr(raster, raster_type), ptr(w, c_f64p), H, W, s, ptr(acc, c_f64p),
                                     ptr(info, c_i64p)))
    return acc, w, s, dict(zip(("rounds", "queue_high", "queued", fourth), (int(v) for v in info)))


def _specific_area(acc, w, s, px):
    """(acc + the cell's own quantised weight) * px, -100 where acc is -100"""
    own = 1.0 if w is None else np.ldexp(np.rint(np.ldexp(w, s)), -s)
    return np.where(acc == -100.0, -100.0, (acc + own) * px)


def weight_frac_bits(weights):
    """The fixed-point scale accumulate_weighted uses by default: the largest s for which every partial sum of the
    quantised weights rint(w * 2^s) over the raster's N cells stays <= 2^52,

        s = 51 - ceil(log2 N) - e,   2^e <= max(weights) < 2^(e+1)

    (so each weight is held to about 52 - ceil(log2 N) significant bits relative to the largest).  All-zero weights
    (and an empty raster) give s = 0.  The weights are validated as accumulate_weighted validates them."""
    d = _weights_f64(weights)
    if d.size == 0:
        return 0
    return _args._default_frac_bits(d.size, float(d.max()))


def accumulate_weighted(fdr, weights, dem=None, frac_bits=None):
    """Weighted flow accumulation: for every cell c, the sum of the weights of the cells strictly upstream of c on
    accumulate's D8 tree (self excluded), as float64.  With weights = 1 it is accumulate(fdr, dem) exactly.

    The weights are summed in int64 fixed point, q = rint(w * 2^s) (round half to even), and the sum is scaled back
    by 2^-s, so the result does not depend on order, tiling or run.  s = frac_bits, by default weight_frac_bits(weights)
    (the finest scale at which no sum can exceed 2^52; then every sum converts to float64 exactly, and a result is
    within n_upstream * 2^-(s+1) of the real sum).  Pass frac_bits=0 for integer weights to get exact integer sums;
    a frac_bits with N * rint(max(weights) * 2^frac_bits) > 2^52 is refused.

    -100 where accumulate(fdr, dem) gives -100: nodata cells (dem <= -100, when dem is given) and cells on a D8
    cycle.  Nodata cells still pass their weight and their inflow downstream, as they pass their count in
    accumulate; give them weight 0 to leave them out.  Weights must be finite and >= 0, of any real or integer dtype
    (integers <= 2^53).  Bad arguments raise ValueError before any library call."""
    f = _args.raster(fdr, "fdr", cap=False, dtype=np.uint8)
    H, W = f.shape
    w = _weights_f64(weights, f.shape)
    d = nodata_mask(dem, f.shape)
    n = H * W
    s = _args.frac_bits(n, float(w.max()) if n else 0.0, frac_bits,
                        " for these weights: N * rint(max(weights) * 2^frac_bits)", "weight_frac_bits gives")
    acc = np.empty((H, W), np.float64)
    check(_lib.lib().dt_flowacc_weighted(ptr(f, c_u8p), ptr(d, c_f32p), ptr(w, c_f64p), H, W, s,
                                         ptr(acc, c_f64p)))
    return acc
