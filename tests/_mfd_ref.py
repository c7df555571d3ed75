"""Pure-numpy reference of descriptools_amd.mfd (multiple-flow-direction shares and contributing area), written from
the definition in that module's docstring, not from the kernels.  Everything is IEEE float64 on the float32 heights;
the one operation that may differ from the GPU's by an ulp is the power with a non-integer exponent.

Conventions (those of tests/_dinf_ref.py): octant k = 0..7 is the neighbour at k pi / 4 counter-clockwise from east,
rows grow to the south (E, NE, N, NW, W, SW, S, SE; D8 codes 1, 128, 64, 32, 16, 8, 4, 2).  Shares are uint16 in
units of 2^-15; eight 0xFFFF mark nodata.  A complete cell sends floor(T * P_k / 2^15) to every receiver but the main
one (largest P, the first of equals) and the rest to the main one."""
import numpy as np

from _dinf_ref import OCT_CODE, OCT_DX, OCT_DY, default_frac_bits, quantise, shift

UNIT = 32768
SQRT2 = 1.4142135623730951
CONTOUR = (0.5, 0.35355339059327373)  # even, odd octants


def flow_shares(dem, exponent=1.1, contour=False, fdr=None):
    """-> uint16[H, W, 8]"""
    z = np.asarray(dem, np.float32)
    H, W = z.shape
    p = float(exponent)
    nod = z <= np.float32(-100)
    valid = np.isfinite(z) & (z > np.float32(-100))
    z64 = np.where(valid, z, 0).astype(np.float64)
    g = np.zeros((8, H, W), np.float64)
    nbv = []
    for k in range(8):
        zk, vk = shift(z64, k, 0.0), shift(valid, k, False)
        nbv.append(vk)
        rec = valid & vk & (zk < z64)
        d = z64 - zk
        g[k] = np.where(rec, d / SQRT2 if k & 1 else d, 0.0)
    rec = g > 0
    gmax = g.max(axis=0)
    has = gmax > 0
    with np.errstate(all="ignore"):
        u = g / np.where(has, gmax, 1.0)
        if p == np.floor(p):
            f = np.ones_like(u)
            for _ in range(int(p)):
                f = f * u
        else:
            f = np.power(u, p)
        if contour:
            for k in range(8):
                f[k] = f[k] * CONTOUR[k & 1]
        f = np.where(rec, f, 0.0)
        F = np.zeros((H, W), np.float64)
        for k in range(8):
            F = F + f[k]
        r = f / np.where(has, F, 1.0)
    main = np.argmax(f, axis=0)  # the first of the largest
    P = np.floor(np.ldexp(r, 15)).astype(np.int64)
    is_main = np.arange(8)[:, None, None] == main[None]
    P[is_main] = 0
    P[is_main] = np.broadcast_to(np.where(has, UNIT - P.sum(axis=0), 0), (8, H, W))[is_main]
    if fdr is not None:
        code = np.asarray(fdr)
        for k in range(8):
            P[k][valid & ~has & (code == OCT_CODE[k]) & nbv[k]] = UNIT
    P[:, nod] = 0xFFFF
    return np.ascontiguousarray(np.moveaxis(P, 0, 2).astype(np.uint16))


def d8_shares(fdr):
    f = np.asarray(fdr)
    s = np.zeros(f.shape + (8,), np.uint16)
    for k, code in enumerate(OCT_CODE):
        s[..., k][f == code] = UNIT
    return s


def check_shares(shares):
    """(P int64[n, 8] with zeros on nodata, nodata bool[n]); ValueError for a word outside the contract"""
    s = np.asarray(shares)
    if s.ndim != 3 or s.shape[2] != 8 or s.dtype != np.uint16:
        raise ValueError("bad share raster")
    flat = s.reshape(-1, 8).astype(np.int64)
    nod = (flat == 0xFFFF).all(axis=1)
    tot = flat.sum(axis=1)
    ok = nod | ((flat <= UNIT).all(axis=1) & ((tot == 0) | (tot == UNIT)))
    if not ok.all():
        raise ValueError("bad shares at flat index %d" % int(np.argmin(ok)))
    flat[nod] = 0
    return flat, nod


def graph(shares):
    """-> (P, nodata, recv, edge, gone): recv[n, 8] the flat index of the neighbour in octant k (clipped), edge[n, 8]
    the share is > 0 and the neighbour lies in the raster and is not nodata, gone[n, 8] the share is > 0 and leaves
    the domain"""
    H, W = np.asarray(shares).shape[:2]
    P, nod = check_shares(shares)
    yy, xx = np.mgrid[0:H, 0:W]
    recv = np.empty((H * W, 8), np.int64)
    edge = np.empty((H * W, 8), bool)
    for k in range(8):
        ny, nx = yy + OCT_DY[k], xx + OCT_DX[k]
        inside = ((ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)).reshape(-1)
        idx = (np.clip(ny, 0, H - 1) * W + np.clip(nx, 0, W - 1)).reshape(-1)
        recv[:, k] = idx
        edge[:, k] = (P[:, k] > 0) & inside & ~nod[idx]
    return P, nod, recv, edge, (P > 0) & ~edge


def split(T, P):
    """what complete cells with totals T[m] and shares P[m, 8] send by octant: floor(T * P_k / 2^15) to every slot but
    the main one, the rest to the main one.  int64 throughout: T <= 2^52, P <= 2^15"""
    T = np.asarray(T, np.int64)
    m = (T[:, None] >> 15) * P + (((T[:, None] & 32767) * P) >> 15)
    rows = np.arange(len(T))
    main = np.argmax(P, axis=1)
    m[rows, main] = 0
    m[rows, main] = T - m.sum(axis=1)
    return m


def accumulate(shares, weights=None, frac_bits=None, full=False):
    """-> float64 raster; full=True: (result, dict(T, q, done, left, edge, gone, nodata, P)) for property tests"""
    H, W = np.asarray(shares).shape[:2]
    n = H * W
    if frac_bits is None:
        wmax = 1.0 if weights is None else (float(np.max(weights)) if n else 0.0)
        frac_bits = default_frac_bits(n, wmax) if n else 0
    q = quantise(weights, (H, W), frac_bits)
    P, nod, recv, edge, gone = graph(shares)
    pending = np.bincount(recv[edge], minlength=n)
    T = q.copy()
    done = np.zeros(n, bool)
    left = 0
    front = np.flatnonzero((pending == 0) & ~nod)
    while front.size:  # Kahn levels
        done[front] = True
        m = split(T[front], P[front])
        e, r = edge[front], recv[front]
        np.add.at(T, r[e], m[e])
        out = gone[front] & e.any(axis=1)[:, None]
        left += int(m[out].sum())
        cand = r[e]
        np.subtract.at(pending, cand, 1)
        front = np.unique(cand[pending[cand] == 0])
    res = np.where(done, np.ldexp((T - q).astype(np.float64), -frac_bits), -100.0).reshape(H, W)
    if full:
        return res, dict(T=T, q=q, done=done, left=left, edge=edge, gone=gone, nodata=nod, P=P)
    return res
