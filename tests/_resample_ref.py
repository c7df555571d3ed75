"""The numpy reference of descriptools_amd.resample, in the association its module docstring states: float64, one
rounding per operation, sums taken in order from 0.  Sequential sums are np.add.accumulate (a plain running sum, unlike
np.sum's pairwise one); a term that the definition skips enters as +0.0, which leaves a running sum that started at
+0.0 unchanged to the bit."""
import numpy as np

METHODS = ("nearest", "bilinear", "cubic", "average", "sum", "min", "max", "mode")


def valid(z):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > -100)


def centres(matrix, shape):
    """(u, v, inside) of the destination centres"""
    a0, a1, a2, b0, b1, b2 = (np.float64(t) for t in matrix)
    Hd, Wd = shape
    x = (np.arange(Wd, dtype=np.float64) + 0.5)[None, :]
    y = (np.arange(Hd, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        u = (a0 + a1 * x) + a2 * y
        v = (b0 + b1 * x) + b2 * y
    return u, v


def _inside(u, v, Hs, Ws):
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)


def _take(z, r, c):
    """z[r, c] with indices outside the raster clipped (the caller masks them), and whether they were inside"""
    Hs, Ws = z.shape
    ok = (r >= 0) & (r < Hs) & (c >= 0) & (c < Ws)
    return z[np.clip(r, 0, Hs - 1), np.clip(c, 0, Ws - 1)], ok


def _kn(t):
    return ((1.5 * t - 2.5) * t) * t + 1.0


def _kf(t):
    return ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0


def _interpolate(z, u, v, cubic):
    """-> (value, has) of a float64 raster at the destination centres"""
    Hs, Ws = z.shape
    ins = _inside(u, v, Hs, Ws)
    u, v = np.where(ins, u, 0.5), np.where(ins, v, 0.5)
    c, r = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    has = ins & valid(z[r, c])
    up, vp = u - 0.5, v - 0.5
    fc, fr = np.floor(up), np.floor(vp)
    c0, r0 = fc.astype(np.int64), fr.astype(np.int64)
    fx, fy = up - fc, vp - fr
    S, D = np.zeros(u.shape), np.zeros(u.shape)
    with np.errstate(all="ignore"):
        for k, wy in enumerate((1.0 - fy, fy)):
            for m, wx in enumerate((1.0 - fx, fx)):
                w = wy * wx
                t, ok = _take(z, r0 + k, c0 + m)
                ok = ok & (w != 0) & valid(t)
                S = np.where(ok, S + w * t, S)
                D = np.where(ok, D + w, D)
        out = S / D
        if cubic:
            wxs = (_kf(1.0 + fx), _kn(fx), _kn(1.0 - fx), _kf(2.0 - fx))
            wys = (_kf(1.0 + fy), _kn(fy), _kn(1.0 - fy), _kf(2.0 - fy))
            whole = np.ones(u.shape, bool)
            acc = np.zeros(u.shape)
            for k in range(4):
                s = np.zeros(u.shape)
                for m in range(4):
                    t, ok = _take(z, r0 - 1 + k, c0 - 1 + m)
                    whole &= ok & valid(t)
                    s = s + wxs[m] * t
                acc = acc + wys[k] * s
            out = np.where(whole, acc, out)
    return out, has


def _spans(e_first, step, n_dst, n_src):
    """per destination index: the edges e0, e1 and the source cells [lo, hi) its interval takes (hi == lo: none)"""
    k = np.arange(n_dst, dtype=np.float64)
    with np.errstate(all="ignore"):
        e0, e1 = e_first + step * k, e_first + step * (k + 1.0)
        some = (e0 < n_src) & (e1 > 0) & (e1 > e0)
        lo = np.where(some, np.floor(np.maximum(e0, 0.0)), 0).astype(np.int64)
        hi = np.where(some, np.ceil(np.minimum(e1, float(n_src))), 0).astype(np.int64)
    hi = np.maximum(hi, lo)
    return e0, e1, lo, hi


def _footprint(e0, e1, lo, hi, n_src):
    """-> (index[n_dst, K], weight[n_dst, K], taken[n_dst, K])"""
    K = max(int((hi - lo).max()), 1)
    idx = lo[:, None] + np.arange(K)[None, :]
    with np.errstate(all="ignore"):
        w = np.minimum(e1[:, None], idx + 1.0) - np.maximum(e0[:, None], idx.astype(np.float64))
        taken = (idx < hi[:, None]) & (w > 0)
    return np.clip(idx, 0, n_src - 1), w, taken


def _area(src, matrix, shape, method, nodata, fill):
    a0, a1, a2, b0, b1, b2 = (np.float64(t) for t in matrix)
    Hs, Ws = src.shape
    Hd, Wd = shape
    C, WX, TX = _footprint(*_spans(a0, a1, Wd, Ws), Ws)
    R, WY, TY = _footprint(*_spans(b0, b2, Hd, Hs), Hs)
    Z = src[R[:, None, :, None], C[None, :, None, :]]  # (Hd, Wd, Ky, Kx)
    taken = TY[:, None, :, None] & TX[None, :, None, :]
    if method == "mode":
        ok = taken if nodata is None else taken & (Z != nodata)
        n = Hd * Wd
        key = (np.arange(n).reshape(Hd, Wd, 1, 1) * 256 + Z)[ok]
        counts = np.bincount(key.reshape(-1), minlength=n * 256).reshape(n, 256)
        best = counts.argmax(axis=1)  # the first maximum: the smallest value
        out = np.where(counts.max(axis=1) > 0, best, fill).astype(np.uint8)
        return out.reshape(Hd, Wd)
    Z64 = Z.astype(np.float64)
    ok = taken & valid(Z64)
    if method in ("min", "max"):
        flat, okf = Z64.reshape(Hd, Wd, -1), ok.reshape(Hd, Wd, -1)
        pad = np.inf if method == "min" else -np.inf
        masked = np.where(okf, flat, pad)
        ext = masked.min(axis=2) if method == "min" else masked.max(axis=2)
        first = (okf & (flat == ext[:, :, None])).argmax(axis=2)  # the first of equal values, in row-major order
        picked = np.take_along_axis(flat, first[:, :, None], axis=2)[:, :, 0]
        return np.where(okf.any(axis=2), picked, -100.0).astype(src.dtype)
    with np.errstate(all="ignore"):
        wx = np.broadcast_to(WX[None, :, None, :], Z64.shape)
        s = np.add.accumulate(np.where(ok, wx * Z64, 0.0), axis=3)[..., -1]
        d = np.add.accumulate(np.where(ok, wx, 0.0), axis=3)[..., -1]
        wy = WY[:, None, :]
        S = np.add.accumulate(np.where(TY[:, None, :], wy * s, 0.0), axis=2)[..., -1]
        D = np.add.accumulate(np.where(TY[:, None, :], wy * d, 0.0), axis=2)[..., -1]
        out = np.where(D > 0, S / D if method == "average" else S, -100.0)
    return out.astype(src.dtype)


def default_fill(dtype):
    return 0 if np.dtype(dtype).kind in "bu" else -100


def warp(src, matrix, shape, method="nearest", nodata=None, fill=None):
    src = np.asarray(src)
    Hs, Ws = src.shape
    shape = (int(shape[0]), int(shape[1]))
    if method in ("nearest", "mode") and fill is None:
        fill = default_fill(src.dtype)
    if method in METHODS[3:]:
        return _area(src, matrix, shape, method, nodata, fill)
    u, v = centres(matrix, shape)
    if method == "nearest":
        ins = _inside(u, v, Hs, Ws)
        c = np.floor(np.where(ins, u, 0.5)).astype(np.int64)
        r = np.floor(np.where(ins, v, 0.5)).astype(np.int64)
        out = np.full(shape, fill, src.dtype)
        out[ins] = src[r[ins], c[ins]]
        return out
    val, has = _interpolate(src.astype(np.float64), u, v, method == "cubic")
    with np.errstate(all="ignore"):
        return np.where(has, val, -100.0).astype(src.dtype)


def resize(src, shape, method="nearest", **kw):
    src = np.asarray(src)
    return warp(src, (0.0, src.shape[1] / shape[1], 0.0, 0.0, 0.0, src.shape[0] / shape[0]), shape, method, **kw)


def aggregate(src, factor, how="average", **kw):
    src = np.asarray(src)
    fy, fx = factor if isinstance(factor, tuple) else (factor, factor)
    shape = (-(-src.shape[0] // fy), -(-src.shape[1] // fx))
    return warp(src, (0.0, float(fx), 0.0, 0.0, 0.0, float(fy)), shape, how, **kw)


RANGE_ZOOM = ((0.0, 0.5, 0.0, 0.0, 0.0, 0.5), (260, 514))


def range_case():
    """The raster of the range checks (test_resample_host.py runs them on this reference, test_gpu_resample.py on the
    library): integer-valued float64 with 5 % nodata.  With an integer factor and the power-of-two zoom RANGE_ZOOM
    every product and sum is exact, S/D rounds once and rounding is monotone, so the ranges hold without slack."""
    rng = np.random.default_rng(11)
    z = rng.integers(-90, 5000, (130, 257)).astype(np.float64)
    z[rng.random(z.shape) < 0.05] = -100.0
    return z


def check_ranges(z, aggregate3, bilinear):
    """min <= average <= max cell by cell on `aggregate3` = (min, average, max) at factor 3, and every value of
    `bilinear` (z through RANGE_ZOOM) within the range of the valid ones of its four taps; none of it looks at how
    the values were made"""
    lo, av, hi = aggregate3
    has = av > -100
    assert has.sum() > 3000 and np.array_equal(has, lo > -100) and np.array_equal(has, hi > -100)
    assert (lo[has] <= av[has]).all() and (av[has] <= hi[has]).all()
    m, shape = RANGE_ZOOM
    u, v = centres(m, shape)
    c0, r0 = np.floor(u - 0.5).astype(int), np.floor(v - 0.5).astype(int)
    tlo, thi = np.full(shape, np.inf), np.full(shape, -np.inf)
    for k in (0, 1):
        for q in (0, 1):
            t, ok = _take(z, r0 + k, np.broadcast_to(c0 + q, shape))
            ok = ok & (t > -100)
            tlo, thi = np.where(ok, np.minimum(tlo, t), tlo), np.where(ok, np.maximum(thi, t), thi)
    has = bilinear > -100
    assert np.array_equal(has, np.repeat(np.repeat(z > -100, 2, 0), 2, 1)), "a value exactly where the containing cell has one"
    assert (bilinear[has] >= tlo[has]).all() and (bilinear[has] <= thi[has]).all()


def same(name, g, r):
    """bit patterns, dtype and shape included"""
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
    gb, rb = g.view(np.uint8), r.view(np.uint8)
    if not np.array_equal(gb, rb):
        bad = np.argwhere((gb != rb).reshape(g.shape + (g.dtype.itemsize,)).any(axis=-1))
        i, j = bad[0]
        raise AssertionError("%s: %d of %d cells differ, first at (%d, %d): %r, reference %r"
                             % (name, len(bad), g.size, i, j, g[i, j], r[i, j]))
