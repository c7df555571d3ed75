"""numpy reference of the threshold curves of descriptools_amd.evaluation (threshold_counts, curve,
calibration_exhaustive, curve_resident and the histogram of dt_threshold_hist behind them), on top of _evaluation_ref.

A cell's classification changes once along a sorted threshold table, at the cell's bin: np.searchsorted on the live
descriptor (R._live: NaN on every cell equal to the first) -- side 'left', the number of thresholds below the value, for
'under', where the cell floods from its bin on; side 'right', the number of thresholds at or below it, otherwise, where
it floods below its bin.  Dead cells (NaN) never flood: bin K / bin 0.  Thresholds are rounded to a float16 / float32
descriptor's dtype first, which is what numpy does with the Python number R.binary_map is given.  test_curve_host.py
pins all of this against R.class_map(R.binary_map(...)) threshold by threshold."""
import collections

import numpy as np

import _evaluation_ref as R

Curve = collections.namedtuple("Curve", "thresholds counts correctness fpr fit tss kappa auc")


def compared(desc, thresholds):
    """the thresholds as float64, rounded to the descriptor's dtype when that is float16 / float32"""
    th = np.asarray(thresholds, np.float64).reshape(-1)
    dt = np.asarray(desc).dtype
    return th.astype(dt).astype(np.float64) if dt in (np.float16, np.float32) else th


def bins(desc, thresholds, under, nodata=None):
    """int64[n]: the bin of every cell.  nodata None: the first-cell rule; else cells equal to `nodata` or NaN are dead
    (the device entries take the nodata value as an argument)"""
    th = compared(desc, thresholds)
    flat = np.asarray(desc).reshape(-1)
    with np.errstate(all="ignore"):
        live = R._live(flat) if nodata is None else np.where(flat == nodata, np.nan, flat.astype(np.float64))
    live = np.asarray(live, np.float64).reshape(-1)
    dead = np.isnan(live)
    j = np.searchsorted(th, np.where(dead, 0.0, live), side="left" if under == "under" else "right")
    return np.where(dead, len(th) if under == "under" else 0, j).astype(np.int64)


def hist(desc, bench, thresholds, under, nodata=None):
    """int64[2 (K + 1) + 1]: bins of the cells whose remapped benchmark value is 0, of those where it is 2, and the
    number of cells with any other benchmark value"""
    K = len(np.asarray(thresholds).reshape(-1))
    j = bins(desc, thresholds, under, nodata)
    g = R.remap(np.asarray(bench).reshape(-1))
    h0 = np.bincount(j[g == 0], minlength=K + 1)
    h2 = np.bincount(j[g == 2], minlength=K + 1)
    return np.concatenate([h0, h2, [np.count_nonzero((g != 0) & (g != 2))]]).astype(np.int64)


def counts_of(h, K, under):
    """int64[K, 4] class counts from the histograms"""
    out = np.empty((K, 4), np.int64)
    for col, part in ((0, h[:K + 1]), (2, h[K + 1:2 * K + 2])):
        upto = np.cumsum(part)[:K]                      # cells of the bins 0..k
        wet = upto if under == "under" else part.sum() - upto
        out[:, col], out[:, col + 1] = part.sum() - wet, wet
    return out


def auc_of(h, K, under):
    """the integer AUC: sum over the bins in flooding order of dry-benchmark cells times (2 x flooded-benchmark cells
    that flood earlier + those of the same bin), over 2 P N; NaN when P N = 0"""
    h0, h2 = [int(v) for v in h[:K + 1]], [int(v) for v in h[K + 1:2 * K + 2]]
    order = range(K + 1) if under == "under" else range(K, -1, -1)
    num = earlier = 0
    for j in order:
        num += h0[j] * (2 * earlier + h2[j])
        earlier += h2[j]
    P, N = sum(h2), sum(h0)
    return num / (2 * P * N) if P * N else float("nan")


def curve_of(thresholds, h, under):
    th = np.array(thresholds, np.float64).reshape(-1)
    K = len(th)
    counts = counts_of(h, K, under)
    c0, c1, c2, c3 = (counts[:, i].astype(np.float64) for i in range(4))
    with np.errstate(all="ignore"):
        tpr, fit = counts[:, 3] / (counts[:, 2] + counts[:, 3]), counts[:, 3] / (counts[:, 3] + counts[:, 2] + counts[:, 1])
        fpr = c1 / (c0 + c1)
        kappa = 2 * (c3 * c0 - c1 * c2) / ((c3 + c1) * (c1 + c0) + (c3 + c2) * (c2 + c0))
    return Curve(th, counts, tpr, fpr, fit, tpr - fpr, kappa, auc_of(h, K, under))


def curve(desc, bench, under, steps=10000, thresholds=None):
    th = np.arange(steps + 1) / steps if thresholds is None else thresholds
    return curve_of(th, hist(desc, bench, th, under), under)


def exhaustive(desc, bench, under, steps=10000, objective="fit"):
    """the lattice threshold with the best objective: NaN is worst, the smallest k wins a tie"""
    score = getattr(curve(desc, bench, under, steps), objective)
    best = None
    for k, s in enumerate(score):
        if s == s and (best is None or s > score[best]):
            best = k
    if best is None:
        raise ValueError("the objective is NaN at every threshold")
    return best / steps


def auc_pairs(desc, bench, under):
    """brute force (Mann-Whitney): over all (benchmark-flooded, benchmark-dry) pairs of cells, 1 when the descriptor
    floods the flooded cell strictly first, 1/2 when they tie; dead cells never flood and tie with each other"""
    live = np.asarray(R._live(np.asarray(desc).reshape(-1)), np.float64)
    key = np.where(np.isnan(live), np.inf, live if under == "under" else -live)  # smaller floods first
    g = R.remap(np.asarray(bench).reshape(-1))
    pos, neg = key[g == 2], key[g == 0]
    if not pos.size * neg.size:
        return float("nan")
    first = int((pos[:, None] < neg[None, :]).sum())
    tie = int((pos[:, None] == neg[None, :]).sum())
    return (2 * first + tie) / (2 * pos.size * neg.size)
