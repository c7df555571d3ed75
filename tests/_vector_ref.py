"""The numpy reference of descriptools_amd/vector.py, written from the module's definitions and not from the kernels:
float64, one rounding per operation, in the association the docstring states.  Polygons: per-edge crossings with
np.repeat, np.lexsort by (row, id, col), pairs -> spans -> np.maximum into the label.  Lines: a Python loop per column of
the major axis.  Geometry is passed as plain arrays (kind, coords, parts, ids), so the reference imports nothing of
the package."""
import numpy as np


def crossings(coords, parts, ids, shape):
    """(row, id, col) of every crossing of a ring edge with a row's centre line, int64 arrays in no particular order"""
    H, W = shape
    coords = np.asarray(coords, np.float64).reshape(-1, 2)
    parts = np.asarray(parts, np.int64)
    ids = np.asarray(ids, np.int64)
    n = np.diff(parts)
    if coords.shape[0] == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    v = np.arange(coords.shape[0])
    part = np.repeat(np.arange(n.size), n)
    nxt = np.where(v + 1 == parts[part + 1], parts[part], v + 1)
    x0, y0, x1, y1 = coords[v, 0], coords[v, 1], coords[nxt, 0], coords[nxt, 1]
    up = y0 <= y1
    xa, ya, xb, yb = np.where(up, x0, x1), np.where(up, y0, y1), np.where(up, x1, x0), np.where(up, y1, y0)
    r0 = np.maximum(np.ceil(ya - 0.5), 0.0)
    r1 = np.minimum(np.ceil(yb - 0.5), float(H))
    cnt = np.where((ya != yb) & (r0 < r1), r1 - r0, 0.0).astype(np.int64)
    e = np.repeat(np.arange(v.size), cnt)
    first = np.cumsum(cnt) - cnt
    row = r0.astype(np.int64)[e] + (np.arange(e.size) - first[e])
    yc = row.astype(np.float64) + 0.5
    t = (yc - ya[e]) / (yb[e] - ya[e])
    x = xa[e] + t * (xb[e] - xa[e])
    col = np.minimum(np.maximum(np.ceil(x - 0.5), 0.0), float(W)).astype(np.int64)
    return row, ids[part][e], col


def count(kind, coords, parts, ids, shape):
    """(total, largest_row) as vector.count_crossings defines them"""
    if kind != "polygon":
        return 0, 0
    row, _, _ = crossings(coords, parts, ids, shape)
    if row.size == 0:
        return 0, 0
    return int(row.size), int(np.bincount(row).max())


def _polygons(label, coords, parts, ids):
    H, W = label.shape
    row, pid, col = crossings(coords, parts, ids, (H, W))
    order = np.lexsort((col, pid, row))
    row, pid, col = row[order], pid[order], col[order]
    assert row.size % 2 == 0
    lo, hi = col[0::2], col[1::2]
    assert (row[0::2] == row[1::2]).all() and (pid[0::2] == pid[1::2]).all(), "an odd count on some (row, id)"
    for r, i, a, b in zip(row[0::2], pid[0::2], lo, hi):
        if a < b:
            np.maximum(label[r, a:b], i, out=label[r, a:b])


def _burn(label, fy, fx, i):
    H, W = label.shape
    if 0.0 <= fy < H and 0.0 <= fx < W:
        label[int(fy), int(fx)] = max(label[int(fy), int(fx)], i)


def _segment(label, xa, ya, xb, yb, i, connectivity):
    H, W = label.shape
    f = np.float64
    xa, ya, xb, yb = f(xa), f(ya), f(xb), f(yb)
    dx, dy = xb - xa, yb - ya
    if dx == 0.0 and dy == 0.0:
        _burn(label, np.floor(ya), np.floor(xa), i)
        return
    if connectivity == 8:
        _burn(label, np.floor(ya), np.floor(xa), i)
        _burn(label, np.floor(yb), np.floor(xb), i)
    xmajor = abs(dx) >= abs(dy)
    ma, na, mb, nb = (xa, ya, xb, yb) if xmajor else (ya, xa, yb, xb)
    if ma > mb:
        ma, na, mb, nb = mb, nb, ma, na
    Wm, Wn = (W, H) if xmajor else (H, W)

    def minor(m):
        if m == ma:
            return na
        if m == mb:
            return nb
        return na + ((m - ma) / (mb - ma)) * (nb - na)

    lo, hi = max(np.floor(ma), f(0.0)), min(np.floor(mb), f(Wm - 1))
    if not lo <= hi:
        return
    for c in range(int(lo), int(hi) + 1):
        if connectivity == 4:
            n1, n2 = minor(max(ma, f(c))), minor(min(mb, f(c) + f(1.0)))
            q0, q1 = max(np.floor(min(n1, n2)), f(0.0)), min(np.floor(max(n1, n2)), f(Wn - 1))
            if q0 <= q1:
                rows = slice(int(q0), int(q1) + 1)
                sel = (rows, c) if xmajor else (c, rows)
                label[sel] = np.maximum(label[sel], i)
        else:
            n = np.floor(minor(min(max(f(c) + f(0.5), ma), mb)))
            if xmajor:
                _burn(label, n, f(c), i)
            else:
                _burn(label, f(c), n, i)


def _lines(label, coords, parts, ids, connectivity, closed):
    for p in range(len(ids)):
        b, e = int(parts[p]), int(parts[p + 1])
        i = int(ids[p])
        if e - b == 1 and not closed:
            _burn(label, np.floor(coords[b, 1]), np.floor(coords[b, 0]), i)
            continue
        last = e if closed else e - 1
        for v in range(b, last):
            w = b if v + 1 == e else v + 1
            _segment(label, coords[v, 0], coords[v, 1], coords[w, 0], coords[w, 1], i, connectivity)


def rasterize(kind, coords, parts, ids, shape, connectivity=8, all_touched=False):
    H, W = shape
    coords = np.asarray(coords, np.float64).reshape(-1, 2)
    parts = np.asarray(parts, np.int64)
    ids = np.asarray(ids, np.int64)
    label = np.full((H, W), -1, np.int64)
    if kind == "polygon":
        _polygons(label, coords, parts, ids)
        if all_touched:
            _lines(label, coords, parts, ids, 4, True)
    elif kind == "line":
        _lines(label, coords, parts, ids, connectivity, False)
    else:
        for p in range(len(ids)):
            for v in range(int(parts[p]), int(parts[p + 1])):
                _burn(label, np.floor(coords[v, 1]), np.floor(coords[v, 0]), int(ids[p]))
    return label.astype(np.int32)


def same(what, got, want):
    """bit for bit, shape and dtype included"""
    assert got.dtype == want.dtype, "%s: dtype %s, expected %s" % (what, got.dtype, want.dtype)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d cells differ, the first at %s: %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
