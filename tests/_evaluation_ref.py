"""numpy reference of descriptools_amd.evaluation, written from the behaviour of the five operations -- scale, binary
map, class map with counts, the two indexes, the four-stage threshold search -- plus the np.unique extremes.

Everything goes through numpy's own dtype promotion: a float16 / float32 raster stays in its dtype beside a Python
number (which is "weak": it is rounded to the raster's dtype first), numpy float scalars promote, integer and bool
rasters become float64 the moment NaN is written into them.  No dtype is special-cased here.

NaN rule of the extremes.  np.unique sorts NaN last, so np.unique(x)[-1] of a raster with one NaN cell is NaN, and a
descriptor with NaN cells could not be scaled.  The kernels skip NaN, and so does extremes(): smallest, second-smallest
distinct and largest of the values that are not NaN; a slot without a value (no second distinct value, no value at
all) is NaN.  -0.0 and +0.0 are one value, as for np.unique; which of the two zeros stands for it is not specified."""
import operator

import numpy as np


def scale(mat, mn, mx, nodata):
    """NaN where mat == nodata or mat is NaN, (mat - mn) / (mx - mn) elsewhere."""
    mat = np.asarray(mat)
    with np.errstate(all="ignore"):
        holed = np.where(mat == nodata, np.nan, mat)  # NaN is weak: float rasters keep their dtype, others -> float64
        return (holed - mn) / (mx - mn)               # NaN cells stay NaN through the arithmetic


def _live(desc):
    """the descriptor with NaN on every cell equal to its first cell (the first-cell rule); ints become float64"""
    desc = np.asarray(desc)
    with np.errstate(all="ignore"):
        return np.where(desc == desc.reshape(-1)[0], np.nan, desc)


def _side(under):
    return operator.le if under == "under" else operator.ge  # any string but 'under' floods upwards


def binary_map(desc, threshold, under):
    """1 on the flooded side of the threshold ('under': <=, any other string: >=), 0 elsewhere, where the descriptor
    is NaN, and on every cell equal to the first cell; int64."""
    with np.errstate(all="ignore"):
        return _side(under)(_live(desc), threshold).astype(np.int64)  # a comparison with NaN is False


def remap(bench):
    """the benchmark map as the class map reads it: 1 -> 2, -100 -> 0, every other value kept; same dtype"""
    bench = np.asarray(bench)
    return np.where(bench == 1, 2, np.where(bench == -100, 0, bench)).astype(bench.dtype)


def _counts(klass):
    flat = np.clip(np.asarray(klass).reshape(-1), -1, 4).astype(np.int64)  # everything outside 0..3 into two bins
    return np.bincount(flat + 1, minlength=6)[1:5]


def class_map(binary, bench):
    """(class map = binary + remapped benchmark map in numpy's promoted dtype, counts of the classes 0..3 BY VALUE).
    0 = both dry, 1 = descriptor only, 2 = benchmark only, 3 = both flooded; other sums are in the map, not counted."""
    klass = np.asarray(binary) + remap(bench)
    return klass, _counts(klass)


def indexes(counts):
    """(correctness, fit): class 3 over the benchmark's flooded cells / over every cell either map floods; NaN for 0/0"""
    c = np.asarray(counts, np.int64)
    with np.errstate(all="ignore"):
        return c[3] / (c[2] + c[3]), c[3] / (c[3] + c[2] + c[1])


def fit_of(desc, bench, under):
    """threshold -> Fit index of the descriptor's map against the benchmark map: indexes(class_map(binary_map(...))[1])
    with what does not depend on the threshold taken once, and the sums counted in int8 (the search asks 61 times).
    Benchmark values are clipped to -2 .. 4 first: with a binary value of 0 or 1 added, a sum is in 0 .. 3 after the
    clipping exactly when it was before."""
    live, side = _live(desc).reshape(-1), _side(under)
    g = np.clip(remap(bench), -2, 4).astype(np.int8).reshape(-1)

    def at(th):
        with np.errstate(all="ignore"):
            return indexes(np.bincount(side(live, th) + g + np.int8(2), minlength=8)[2:6])[1]
    return at


# the refinement stages after the coarse pick: thresholds (centre - half .. centre + half) / divisor in `step`s; a
# candidate replaces the best so far when better(fit, best).  Only the first stage lets an equal fit win.
STAGES = ((100, 20, 10, operator.ge),
          (100, 5, 1, operator.gt),
          (1000, 10, 1, operator.gt),
          (10000, 10, 1, operator.gt))


def search(fit_at, stages=STAGES):
    """The four-stage search for the threshold of the best fit.  fit_at(threshold) -> fit.  Coarse pick among
    0.25 / 0.50 / 0.75: the larger of the upper two (0.50 on a tie) if it beats 0.25, else 0.25.  Every comparison
    with a NaN fit is False, so a search in which no candidate of the first stage reaches the coarse fit has no
    threshold: UnboundLocalError, which is what the original's unassigned local raises."""
    f25, f50, f75 = (fit_at(i / 100) for i in (25, 50, 75))
    centre, best = (75, f75) if f75 > f50 else (50, f50)
    if not best > f25:
        centre, best = 25, f25
    pick, prev = None, 100
    for k, (div, half, step, better) in enumerate(stages):
        if k:
            if pick is None:
                raise UnboundLocalError("no threshold: the fit is NaN at every first-stage candidate")
            centre = pick = pick * (div // prev)
        for i in range(centre - half, centre + half + 1, step):
            f = fit_at(i / div)
            if better(f, best):
                best, pick = f, i
        prev = div
    return pick / 10000


def calibrate(desc, bench, under):
    return search(fit_of(desc, bench, under))


def extremes(x):
    """(smallest, second-smallest distinct, largest) of the non-NaN values of x, in x's dtype; NaN for a missing slot
    (the NaN rule in the module docstring)."""
    x = np.asarray(x).reshape(-1)
    u = np.unique(x[~np.isnan(x)])
    out = np.full(3, np.nan, x.dtype)
    if u.size:
        out[0], out[2] = u[0], u[-1]
    if u.size > 1:
        out[1] = u[1]
    return out


def same(a, b):
    """equal values, equal dtype and shape, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
