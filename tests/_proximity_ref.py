"""numpy reference of descriptools_amd.proximity (the definition in that module's docstring), in two independent forms.

brute(river, nodata): d2 of every cell against every source, the sources listed in row-major order, argmin (whose
first-of-equals is the tie rule: the smallest flat index); chunked over cells, so memory stays bounded.
sweep(river, nodata): the nearest source of each row (left on ties), then for y' ascending `best` is replaced where
(y - y')^2 + f[y'] is STRICTLY smaller; O(H) vectorised steps, usable up to ~500 rows.

Both return (indices int64, distance float32, d2 int64), -100 on nodata and when there is no source; distance is the
definition's float32(px * sqrt(float64(d2)))."""
import numpy as np

SENTINEL = 1 << 62


def sources(river, nodata=None):
    src = np.asarray(river) == 1
    if nodata is not None:
        src &= ~np.asarray(nodata, bool)
    return src


def distance(d2, px):
    d2 = np.asarray(d2)
    with np.errstate(invalid="ignore"):
        d = (float(px) * np.sqrt(d2.astype(np.float64))).astype(np.float32)
    return np.where(d2 < 0, np.float32(-100), d)


def _finish(idx, d2, nodata, px):
    if nodata is not None:
        nd = np.asarray(nodata, bool)
        idx[nd] = -100
        d2[nd] = -100
    return idx, distance(d2, px), d2


def brute(river, nodata=None, px=1.0, chunk_elems=1 << 22):
    src = sources(river, nodata)
    H, W = src.shape
    idx = np.full((H, W), -100, np.int64)
    d2 = np.full((H, W), -100, np.int64)
    flat = np.flatnonzero(src.reshape(-1))  # ascending flat index: row-major order
    if flat.size:
        sy, sx = np.divmod(flat, W)
        step = max(1, chunk_elems // flat.size)
        fi, fd = idx.reshape(-1), d2.reshape(-1)
        for c0 in range(0, H * W, step):
            cy, cx = np.divmod(np.arange(c0, min(c0 + step, H * W), dtype=np.int64), W)
            d = (cy[:, None] - sy[None, :]) ** 2 + (cx[:, None] - sx[None, :]) ** 2
            k = np.argmin(d, axis=1)  # the first of equals
            fi[c0:c0 + len(k)] = flat[k]
            fd[c0:c0 + len(k)] = d[np.arange(len(k)), k]
    return _finish(idx, d2, nodata, px)


def row_nearest(src):
    """per cell the column of the nearest source of its own row, the left one of two equally far, -1 without one"""
    H, W = src.shape
    cols = np.arange(W, dtype=np.int64)
    left = np.maximum.accumulate(np.where(src, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(src, cols, W + W)[:, ::-1], axis=1)[:, ::-1]
    none_r = right >= W + W
    take_left = (left >= 0) & (none_r | (cols - left <= right - cols))
    return np.where(take_left, left, np.where(none_r, -1, right))


def sweep(river, nodata=None, px=1.0):
    src = sources(river, nodata)
    H, W = src.shape
    cx = row_nearest(src)
    f = np.where(cx >= 0, (np.arange(W, dtype=np.int64) - cx) ** 2, SENTINEL)
    yy = np.arange(H, dtype=np.int64)[:, None]
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    arow = np.zeros((H, W), np.int64)
    for y1 in range(H):
        cost = (yy - y1) ** 2 + f[y1][None, :]
        better = cost < best
        best[better] = cost[better]
        arow[better] = y1
    found = best < SENTINEL
    idx = np.where(found, arow * W + np.take_along_axis(cx, arow, axis=0), -100)
    d2 = np.where(found, best, -100)
    return _finish(idx, d2, nodata, px)
