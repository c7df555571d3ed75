"""Flood-map evaluation -- replacement of descriptools/evaluation.py.

Every raster-returning function is an H2D -> kernel -> D2H shim like the other modules: `minMaxScale`
(k_minmax_scale_den, float16: k_minmax_scale_h), `binary_map` and `avaliacao` (k_classify).  `calibration` -- 61 x
(binary_map + avaliacao) in the reference -- runs as 5 multi-threshold confusion-count passes over rasters uploaded
once (k_confusion); counts are exact integers, so the returned threshold is identical.  The numpy dtype rules of the
reference's expressions are kept at the boundary (which arithmetic a float16 / float32 / integer raster is scaled and
compared in, Python numbers rounded to the raster's dtype as numpy's weak scalars are, int64 maps out,
the in-place remap of the benchmark map).

Net-new beside the reference's functions: `threshold_counts`, `curve`, `calibration_exhaustive` and `curve_resident` --
the confusion counts at every threshold of a sorted table from one pass (k_threshold_hist), and from them the ROC curve,
its area, and the best threshold of the whole lattice k / steps instead of the four-stage search's 61 samples of it."""
import collections

import numpy as np

from . import _lib
from ._lib import C, c_f64p, c_i8p, c_i32p, c_i64p, c_u8p, check, ptr
from .device import Context


def _float_view(mat, *scalars):
    """(contiguous float array, its dtype): the float dtype numpy's expressions give a raster of this dtype when
    combined with `scalars` -- float16 and float32 rasters keep their dtype beside Python numbers (which are weak)
    and are promoted by numpy float scalars, every other dtype is computed in float64."""
    mat = np.asarray(mat)
    base = mat.dtype if mat.dtype in (np.float16, np.float32) else np.float64
    rt = np.result_type(base, *scalars)
    rt = np.dtype(rt if rt in (np.float16, np.float32) else np.float64)
    return np.ascontiguousarray(mat, rt), rt


def _weak(value, raster_dtype, rt):
    """the scalar as numpy compares it with a float raster computed in `rt`: rounded to the raster's dtype if it is a
    Python number, promoted (compared exactly) if it is a numpy scalar -- NaN, which equals nothing, when the exact
    comparison value is not a value of `rt`"""
    if np.dtype(raster_dtype).kind != 'f':
        return float(value)
    with np.errstate(over='ignore'):
        v = np.asarray(value).astype(np.result_type(raster_dtype, value))
        return float(v) if float(v.astype(rt)) == float(v) or v != v else float('nan')


def _float_dtype(*args):
    rt = np.result_type(*args)
    return np.dtype(rt if rt in (np.float16, np.float32) else np.float64)


def _scale_call(x, mn, den, nodata):
    out = np.empty_like(x)
    check(_lib.lib().dt_minmax_scale_den(x.ctypes.data_as(C.c_void_p), x.dtype.itemsize, x.size, mn, den, nodata,
                                         out.ctypes.data_as(C.c_void_p)))
    return out


def minMaxScale(mat, mn, mx, nodata):
    """evaluation.py:5-9 on the GPU: NaN where mat == nodata (or mat is NaN), (mat - mn) / (mx - mn) elsewhere, in
    numpy's dtypes: the difference in the dtype the raster and mn give, the denominator subtracted between the scalars
    themselves and then rounded to the result's dtype, float16 rasters scaled in float16 beside Python numbers."""
    mat = np.asarray(mat)
    with np.errstate(over='ignore', invalid='ignore'):
        den = mx - mn
        dt_diff = _float_dtype(mat.dtype if mat.dtype.kind == 'f' else np.float64, mn)
        rt = _float_dtype(dt_diff, den)
        mn_v, den_v = float(np.asarray(mn).astype(dt_diff)), float(np.asarray(den).astype(rt))
    x = np.ascontiguousarray(mat, dt_diff)
    nod = _weak(nodata, mat.dtype, dt_diff)
    if dt_diff == rt:
        return _scale_call(x, mn_v, den_v, nod)
    # the difference is rounded in its own dtype and widened for the division: (x - mn) / 1, then (d - 0) / den, exact
    return _scale_call(_scale_call(x, mn_v, 1.0, nod).astype(rt), 0.0, den_v, float('nan'))


def _compare_view(descriptor_matrix, threshold):
    """(contiguous float32 / float64 raster, is_f32, threshold) for the comparison kernels: a float16 raster is compared
    on its exactly widened float32 values with the threshold numpy would use -- rounded to float16 when it is a Python
    number"""
    desc, rt = _float_view(descriptor_matrix, threshold)
    if rt == np.float16:
        with np.errstate(over='ignore'):
            return desc.astype(np.float32), True, float(np.float16(threshold))
    return desc, rt == np.float32, float(threshold)


def binary_map(descriptor_matrix, threshold, under):
    """evaluation.py:90-123 on the GPU; int64 map out; the value at [0, 0] counts as nodata (:111)."""
    desc, is_f32, threshold = _compare_view(descriptor_matrix, threshold)
    first = float(desc.reshape(-1)[0]) if desc.size else 0.0
    out = np.empty(desc.shape, np.uint8)
    check(_lib.lib().dt_binary_map(desc.ctypes.data_as(C.c_void_p), int(is_f32), desc.size, first, threshold,
                                   1 if under == 'under' else 0, ptr(out, c_u8p)))
    return out.astype(np.int64)


def correctness(count):
    """evaluation.py:174-191: share of the benchmark's flooded cells the descriptor map also floods,
    class 3 / (class 2 + class 3)."""
    hit, miss = count[3], count[2]
    return hit / (miss + hit)


def fit(count):
    """evaluation.py:194-211: class 3 over every cell either map floods."""
    hit, miss, false_alarm = count[3], count[2], count[1]
    return hit / (hit + miss + false_alarm)


def avaliacao(descriptor_flood_map, comparison_flood_map):
    """evaluation.py:126-171 on the GPU.  Like the reference it rewrites comparison_flood_map in place
    (1 -> 2, -100 -> 0: the kernel's remapped copy is written back into the caller's array); returns
    (correctness, fit, class map = descriptor map + remapped benchmark map).  The classes are counted by value
    (cells whose sum is 0, 1, 2, 3); the reference counts by position in np.unique's output, which is undefined on maps
    whose sums leave 0..3 (a benchmark value other than -100, 0, 1), so only the class map is comparable there."""
    b32 = np.ascontiguousarray(descriptor_flood_map, np.int32)
    cmp8 = np.ascontiguousarray(comparison_flood_map, np.int8)
    klass = np.empty(b32.shape, np.int32)
    counts = np.zeros(4, np.int64)
    check(_lib.lib().dt_avaliacao(ptr(b32, c_i32p), ptr(cmp8, c_i8p), b32.size, ptr(klass, c_i32p),
                                  ptr(counts, c_i64p)))
    comparison_flood_map[...] = cmp8.reshape(np.shape(comparison_flood_map))
    result = klass.astype(np.result_type(np.asarray(descriptor_flood_map).dtype,
                                         np.asarray(comparison_flood_map).dtype))
    with np.errstate(divide='ignore', invalid='ignore'):
        return correctness(counts), fit(counts), result


class _Calibrator:
    """descriptor + benchmark resident on the GPU; one launch per calibration stage."""

    def __init__(self, descriptor_matrix, comparison_matrix, under):
        desc = np.asarray(descriptor_matrix)
        # numpy compares a float32 / float16 raster with a Python float in the raster's dtype
        self.round_to = desc.dtype.type if desc.dtype in (np.float16, np.float32) else None
        self.nodata = float(desc.reshape(-1)[0]) if desc.size else 0.0
        d64 = np.ascontiguousarray(desc, np.float64)
        cmp8 = np.ascontiguousarray(comparison_matrix, np.int8)
        self.n = d64.size
        self.under = 1 if under == 'under' else 0
        self.ctx = Context()
        self.d_desc = self.ctx.to_device(d64)
        self.d_cmp = self.ctx.to_device(cmp8)
        self.d_counts = self.ctx.empty(24 * 4, np.int64)

    def fits(self, thresholds):
        th = np.asarray(thresholds, np.float64)
        if self.round_to is not None:
            th = th.astype(self.round_to).astype(np.float64)
        th = np.ascontiguousarray(th)
        check(_lib.lib().dt_dev_confusion_multi(self.ctx.h, self.d_desc.ptr, self.d_cmp.ptr, self.n,
                                                self.nodata, ptr(th, c_f64p), len(th), self.under,
                                                self.d_counts.ptr))
        counts = self.d_counts.to_host()[:4 * len(th)].reshape(len(th), 4)
        with np.errstate(divide='ignore', invalid='ignore'):
            return [fit(c) for c in counts]

    def remap_into(self, comparison_matrix):
        """the benchmark map remapped on the device (1 -> 2, -100 -> 0, evaluation.py:149-150) and copied back
        into the caller's array, which the reference's first avaliacao call mutates"""
        check(_lib.lib().dt_dev_classify(self.ctx.h, self.d_desc.ptr, self.d_cmp.ptr, self.n, self.nodata, 0.0,
                                         self.under, 1, None, None, self.d_counts.ptr))
        np.copyto(comparison_matrix, self.d_cmp.to_host().reshape(np.shape(comparison_matrix)), casting='unsafe')

    def close(self):
        for b in (self.d_desc, self.d_cmp, self.d_counts):
            b.free()
        self.ctx.close()


def _grid_search(fits):
    """evaluation.py:12-87: the 4-stage grid search, given fits(list of thresholds) -> list of Fit indexes."""
    f1, f2, f3 = fits([25 / 100, 50 / 100, 75 / 100])
    if f3 > f2:
        fit_index, iteration_value = (f3, 75) if f3 > f1 else (f1, 25)
    else:
        fit_index, iteration_value = (f2, 50) if f2 > f1 else (f1, 25)
    rng = list(range(iteration_value - 20, iteration_value + 30, 10))
    for i, f in zip(rng, fits([i / 100 for i in rng])):
        if f >= fit_index:
            fit_index, threshold = f, i
    iteration_value = threshold
    rng = list(range(iteration_value - 5, iteration_value + 6, 1))
    for i, f in zip(rng, fits([i / 100 for i in rng])):
        if f > fit_index:
            fit_index, threshold = f, i
    for div in (1000, 10000):
        iteration_value = threshold * 10
        threshold = iteration_value
        rng = list(range(iteration_value - 10, iteration_value + 11, 1))
        for i, f in zip(rng, fits([i / div for i in rng])):
            if f > fit_index:
                fit_index, threshold = f, i
    return threshold / 10000


def calibration(descriptor_matrix, comparison_matrix, under):
    """evaluation.py:12-87: 4-stage grid search for the threshold maximising the Fit index."""
    cal = _Calibrator(descriptor_matrix, comparison_matrix, under)
    try:
        cal.remap_into(comparison_matrix)
        return _grid_search(cal.fits)
    finally:
        cal.close()


# ---- threshold curves (net-new) ----------------------------------------------------------------------
CURVE_K_MAX = 65535

Curve = collections.namedtuple("Curve", "thresholds counts correctness fpr fit tss kappa auc")
Curve.__doc__ = """One descriptor against one benchmark map at K sorted thresholds.  thresholds: float64[K] as given;
counts: int64[K, 4], the classes 0..3 of avaliacao (both dry, descriptor only, benchmark only, both flooded);
correctness (the true-positive rate), fpr, fit, tss (correctness - fpr) and kappa (Cohen's): float64[K] quotients of
those integers, NaN for 0/0; auc: the area under (fpr, correctness) closed to (0, 0) and (1, 1), ties counted half."""


def _curve_thresholds(thresholds, round_to):
    """float64[K] as the kernel compares them: rounded to a float16 / float32 descriptor's dtype first (numpy's weak
    Python scalars, as _Calibrator.fits), then checked -- ValueError for a count outside 1..65535, a NaN, a descent"""
    th = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
    if not 1 <= th.size <= CURVE_K_MAX:
        raise ValueError("%d thresholds: a curve takes 1 to %d" % (th.size, CURVE_K_MAX))
    if np.isnan(th).any():
        raise ValueError("threshold %d is NaN" % int(np.argmax(np.isnan(th))))
    if round_to is not None:
        with np.errstate(over='ignore'):
            th = th.astype(round_to).astype(np.float64)
    if not (th[:-1] <= th[1:]).all():
        k = int(np.argmin(th[:-1] <= th[1:]))
        raise ValueError("thresholds are not sorted ascending: %r at %d is followed by %r" % (th[k], k, th[k + 1]))
    return th


def _hist_counts(hist, K, under):
    """int64[K, 4] from the two bin histograms (dt_threshold_hist): a cell of bin j floods at every k >= j ('under') or
    at every k < j, so the flooded cells at k are a prefix sum; ValueError when the extra counter is not 0"""
    hist = np.asarray(hist, np.int64)
    if hist[2 * K + 2]:
        raise ValueError("%d cells of the benchmark map hold a value other than -100, 0 and 1" % int(hist[2 * K + 2]))
    counts = np.empty((K, 4), np.int64)
    for col, h in ((0, hist[:K + 1]), (2, hist[K + 1:2 * K + 2])):
        below = np.cumsum(h)[:K]
        wet = below if under else h.sum() - below
        counts[:, col], counts[:, col + 1] = h.sum() - wet, wet
    return counts


def _hist_auc(hist, K, under):
    """num / (2 P N) in Python integers, num = sum_j h0[j] (2 S2(j) + h2[j]) with S2(j) the benchmark-flooded cells in
    the bins that flood before bin j: every (flooded, dry) pair of benchmark cells counts 2 when the descriptor floods
    the flooded one first and 1 when both flood at the same threshold.  NaN when P N = 0."""
    h0 = [int(v) for v in hist[:K + 1]]
    h2 = [int(v) for v in hist[K + 1:2 * K + 2]]
    if not under:
        h0.reverse()
        h2.reverse()
    num = before = 0
    for a, b in zip(h0, h2):
        num += a * (2 * before + b)
        before += b
    den = 2 * before * sum(h0)
    return num / den if den else float('nan')


def _curve_of(thresholds, hist, under):
    K = len(thresholds)
    counts = _hist_counts(hist, K, under)
    c0, c1, c2, c3 = (counts[:, i].astype(np.float64) for i in range(4))
    with np.errstate(divide='ignore', invalid='ignore'):
        tpr, fpr = correctness(counts.T), c1 / (c0 + c1)
        kappa = 2 * (c3 * c0 - c1 * c2) / ((c3 + c1) * (c1 + c0) + (c3 + c2) * (c2 + c0))
        return Curve(np.array(thresholds, np.float64), counts, tpr, fpr, fit(counts.T), tpr - fpr, kappa,
                     _hist_auc(hist, K, under))


def _threshold_hist(descriptor_matrix, comparison_matrix, thresholds, under):
    """(thresholds as compared, the histograms of dt_threshold_hist) of a host descriptor against a host benchmark map"""
    desc = np.asarray(descriptor_matrix)
    if desc.shape != np.shape(comparison_matrix):
        raise ValueError("the descriptor has shape %s, the benchmark map %s" % (desc.shape, np.shape(comparison_matrix)))
    th = _curve_thresholds(thresholds, desc.dtype.type if desc.dtype in (np.float16, np.float32) else None)
    nodata = float(desc.reshape(-1)[0]) if desc.size else 0.0
    d64 = np.ascontiguousarray(desc, np.float64)
    cmp8 = np.ascontiguousarray(comparison_matrix, np.int8)
    # the kernel remaps 1 -> 2 as avaliacao does and so takes a raw 2 for a flooded cell; a value beyond int8 would wrap
    if (cmp8 == 2).any() or not np.array_equal(cmp8, comparison_matrix):
        raise ValueError("the benchmark map holds a value other than -100, 0 and 1")
    hist = np.empty(2 * (len(th) + 1) + 1, np.int64)
    check(_lib.lib().dt_threshold_hist(ptr(d64, c_f64p), ptr(cmp8, c_i8p), d64.size, nodata, ptr(th, c_f64p), len(th),
                                       1 if under == 'under' else 0, ptr(hist, c_i64p)))
    return th, hist


def threshold_counts(descriptor_matrix, comparison_matrix, thresholds, under):
    """int64[K, 4]: the class counts 0..3 that avaliacao(binary_map(descriptor_matrix, t, under), comparison_matrix)
    counts, for every t of the ascending `thresholds` (1 to 65535 of them), from one pass over the rasters
    (k_threshold_hist).  As in binary_map the descriptor's first cell is its nodata, and a float16 / float32 descriptor
    compares with the thresholds rounded to its dtype.  comparison_matrix is left as it is.  ValueError for thresholds
    that are unsorted or NaN, for rasters of different shapes, for a benchmark value outside {-100, 0, 1}."""
    th, hist = _threshold_hist(descriptor_matrix, comparison_matrix, thresholds, under)
    return _hist_counts(hist, len(th), under == 'under')


def curve(descriptor_matrix, comparison_matrix, under, steps=10000, thresholds=None):
    """The Curve of a scaled descriptor against a benchmark map at `thresholds` (default: the lattice k / steps,
    k = 0..steps, that `calibration` searches a part of); the rules of threshold_counts."""
    if thresholds is None:
        thresholds = np.arange(int(steps) + 1) / int(steps)
    given = np.array(thresholds, np.float64).reshape(-1)
    _, hist = _threshold_hist(descriptor_matrix, comparison_matrix, given, under)
    return _curve_of(given, hist, under == 'under')


CURVE_OBJECTIVES = ("fit", "tss", "kappa")


def calibration_exhaustive(descriptor_matrix, comparison_matrix, under, steps=10000, objective="fit"):
    """The threshold k / steps, k = 0..steps, with the largest Fit index ("fit"), true skill statistic ("tss") or Cohen's
    kappa ("kappa"); the smallest such k on a tie, NaN counting as worst, ValueError when the objective is NaN at every
    k.  With steps = 10000 the lattice holds every threshold in [0, 1] that `calibration`'s four-stage search can
    return, so this Fit is never below that one's.  comparison_matrix is left as it is."""
    if objective not in CURVE_OBJECTIVES:
        raise ValueError("objective must be one of %s, not %r" % (CURVE_OBJECTIVES, objective))
    if int(steps) < 1:
        raise ValueError("steps must be at least 1")
    c = curve(descriptor_matrix, comparison_matrix, under, steps=steps)
    score = getattr(c, objective)
    if np.isnan(score).all():
        raise ValueError("the %s objective is NaN at every threshold" % objective)
    return int(np.argmax(np.where(np.isnan(score), -np.inf, score))) / int(steps)


def curve_resident(ctx, desc_ptr, flood_ptr, n, thresholds, under, nodata_value, reduce_hist=None):
    """The Curve of rasters that are already in HBM: desc the scaled float64 descriptor that
    evaluate_resident(desc_ptr=...) leaves behind, flood the int8 benchmark map, both flat device pointers of n cells.
    thresholds are compared in float64 as given (evaluate_resident rounds its own to float32 for a raster scaled in
    float32).  nodata_value: the scaled value at global cell [0, 0], as evaluate_resident's nodata_first.
    reduce_hist(int64 array) -> int64 array hooks in the sum all-reduce of a multi-rank run: the histograms are
    integers, so every rank gets the whole raster's curve.  ValueError for a benchmark value the kernel does not know
    (it knows -100, 0, 1 and, like k_confusion, takes a raw 2 for what 1 is remapped to)."""
    th = _curve_thresholds(thresholds, None)
    d_th, d_hist = ctx.to_device(th), ctx.empty(2 * (len(th) + 1) + 1, np.int64)
    try:
        check(_lib.lib().dt_dev_threshold_hist(ctx.h, desc_ptr, flood_ptr, n, float(nodata_value), d_th.ptr, len(th),
                                               1 if under == 'under' else 0, d_hist.ptr))
        hist = d_hist.to_host()
    finally:
        d_th.free()
        d_hist.free()
    if reduce_hist is not None:
        hist = np.asarray(reduce_hist(hist), np.int64)
    return _curve_of(th, hist, under == 'under')


def combine_extremes(per_rank):
    """np.unique extremes of a raster split over ranks from each rank's (smallest, second-smallest
    distinct, largest): the global second-smallest is the smallest candidate above the global minimum.  NaN cells are
    no values (dt_dev_unique_extremes_f32 skips them): a rank's slot is NaN when it has no such value, and so is the
    result's."""
    a = np.asarray(per_rank, np.float64).reshape(-1, 3)
    if np.isnan(a[:, 0]).all():  # no rank holds a value
        return np.full(3, np.nan, np.float32)
    lo = np.nanmin(a[:, 0])
    cand = np.where(a[:, 0] > lo, a[:, 0], a[:, 1])
    return np.array([lo, np.nan if np.isnan(cand).all() else np.nanmin(cand), np.nanmax(a[:, 2])], np.float32)


def evaluate_resident(ctx, x_ptr, flood_ptr, n, under='under', nodata=-100.0, desc_ptr=None,
                      reduce_extremes=None, reduce_counts=None, nodata_first=None, integer_valued=False,
                      binary_ptr=None, class_ptr=None, remap_flood=False):
    """Example/example.py:113-147 on rasters that are already in HBM (net-new):
    np.unique extremes -> minMaxScale -> calibration -> confusion counts at the calibrated threshold.
    x is a float32 descriptor raster (e.g. the chain's HAND), flood an int8 benchmark map, both flat
    device pointers of n cells.  reduce_extremes(np.float32[3]) / reduce_counts(np.int64[k, 4]) hook in
    the extremes combination (combine_extremes over an all-gather) and the sum all-reduce of a multi-GPU
    run; nodata_first = the scaled value at global cell [0, 0] (binary_map's nodata, evaluation.py:111)
    when this rank does not own that cell.  integer_valued: x holds integers (the example's int16 HAND kept as
    float32 on the device), which numpy scales and compares in float64 (float32 otherwise).  binary_ptr (uint8[n])
    / class_ptr (int32[n]): device rasters that receive binary_map's map and avaliacao's class map at the
    calibrated threshold (Example/example.py:139-147, what example.py:201-217 writes to disk); remap_flood: the
    benchmark map is left remapped in place as avaliacao leaves it.  Returns a dict."""
    import ctypes as C
    L = _lib.lib()
    own_desc = None
    ext = ctx.empty(3, np.float32)
    counts = ctx.empty(24 * 4, np.int64)
    try:
        check(L.dt_dev_unique_extremes_f32(ctx.h, x_ptr, n, ext.ptr))
        e = ext.to_host()
        if reduce_extremes is not None:
            e = reduce_extremes(e)
        lo, mn, mx = (np.float32(v) for v in e)
        if desc_ptr is None:
            own_desc = ctx.empty(n, np.float64)
            desc_ptr = own_desc.ptr
        if integer_valued:
            check(L.dt_dev_minmax_scale_f32_f64(ctx.h, x_ptr, n, float(mn), float(mx), float(nodata), desc_ptr))
        else:
            check(L.dt_dev_minmax_scale_f32(ctx.h, x_ptr, n, mn, mx, np.float32(nodata), desc_ptr))
        # binary_map treats the value at [0, 0] as nodata (evaluation.py:111); after minMaxScale that is
        # NaN wherever the first cell is nodata -- NaN never compares equal, so pass NaN
        first = np.empty(1, np.float64)
        check(L.dt_dev_d2h(ctx.h, first.ctypes.data_as(C.c_void_p), desc_ptr, 8))
        # (a callable nodata_first is evaluated here, after the extremes are known: a rank that does not own the
        # global cell [0, 0] learns its scaled value with the extremes exchange)
        nod_val = float(first[0]) if nodata_first is None else (nodata_first() if callable(nodata_first) else nodata_first)
        under_i = 1 if under == 'under' else 0

        def count(ths):
            # a float32 descriptor compares with the thresholds in float32 (numpy's weak Python scalars)
            th = np.asarray(ths, np.float64)
            if not integer_valued:
                th = th.astype(np.float32).astype(np.float64)
            th = np.ascontiguousarray(th)
            check(L.dt_dev_confusion_multi(ctx.h, desc_ptr, flood_ptr, n, nod_val, ptr(th, c_f64p), len(th),
                                           under_i, counts.ptr))
            c = counts.to_host()[:4 * len(th)].reshape(len(th), 4).copy()
            return reduce_counts(c) if reduce_counts is not None else c

        def fits(ths):
            with np.errstate(divide='ignore', invalid='ignore'):
                return [fit(c) for c in count(ths)]

        th = _grid_search(fits)
        if binary_ptr is not None or class_ptr is not None or remap_flood:
            thc = float(th) if integer_valued else float(np.float32(th))
            check(L.dt_dev_classify(ctx.h, desc_ptr, flood_ptr, n, nod_val, thc, under_i, 1 if remap_flood else 0,
                                    binary_ptr, class_ptr, counts.ptr))
            c4 = counts.to_host()[:4].copy()
            if reduce_counts is not None:
                c4 = reduce_counts(c4.reshape(1, 4))[0]
        else:
            c4 = count([th])[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            return {"mn": float(mn), "mx": float(mx), "threshold": th, "counts": c4,
                    "correctness": correctness(c4), "fit": fit(c4)}
    finally:
        ext.free()
        counts.free()
        if own_desc is not None:
            own_desc.free()
