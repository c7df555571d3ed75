"""Pure-numpy reference of descriptools_amd.dinf (D-infinity flow direction and contributing area), written from the
definition in that module's docstring and from Tarboton (1997), not from any other program's source.  Everything is
IEEE float64 unless said otherwise; the one operation that may differ from the GPU's by an ulp is arctan2.

Conventions: angle in radians counter-clockwise from east, rows grow to the south; octant k = 0..7 is the neighbour at
k pi / 4 (E, NE, N, NW, W, SW, S, SE; D8 codes 1, 128, 64, 32, 16, 8, 4, 2).  Nodata is z <= -100, which includes
-inf (the package's rule); NaN and +inf are the non-finite centres that get -1 / 0.  A complete cell with two
receivers sends m2 = floor(T * P2 / 2^30) to octant k + 1 (the one that holds share P2) and T - m2 to octant k."""
import math

import numpy as np

OCT_DY = (0, -1, -1, -1, 0, 1, 1, 1)
OCT_DX = (1, 1, 0, -1, -1, -1, 0, 1)
OCT_CODE = (1, 128, 64, 32, 16, 8, 4, 2)
# (e1 octant, e2 octant, ac, af), facets 1..8
FACETS = ((0, 1, 0, 1), (2, 1, 1, -1), (2, 3, 1, 1), (4, 3, 2, -1), (4, 5, 2, 1), (6, 5, 3, -1), (6, 7, 3, 1),
          (0, 7, 4, -1))
PI = math.pi
F2PI = np.float32(2.0 * PI)
FOUR_OVER_PI = 1.2732395447351628
SNAP = 2.0 ** -20
ONE = 1 << 30


def shift(a, k, fill):
    """out[y, x] = a[y + dy_k, x + dx_k], `fill` where that lies outside the raster"""
    H, W = a.shape
    out = np.full((H, W), fill, a.dtype)
    dy, dx = OCT_DY[k], OCT_DX[k]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def octant_angle(k):
    return np.float32(k * PI / 4)


def d8_angles(fdr):
    """float32(k pi / 4) for the eight D8 codes, -1 elsewhere"""
    a = np.full(fdr.shape, -1, np.float32)
    for k, code in enumerate(OCT_CODE):
        a[fdr == code] = octant_angle(k)
    return a


def flow_direction(dem, px, fdr=None):
    """-> (angle float32, slope float32)"""
    z = np.asarray(dem, np.float32)
    H, W = z.shape
    px = float(px)
    nod = z <= np.float32(-100)
    valid = np.isfinite(z) & (z > np.float32(-100))
    z64 = np.where(valid, z, 0).astype(np.float64)
    nb = [shift(z64, k, 0.0) for k in range(8)]
    nbv = [shift(valid, k, False) for k in range(8)]
    best = np.zeros((H, W), np.float64)
    ang = np.zeros((H, W), np.float64)
    won = np.zeros((H, W), bool)
    pxd = px * np.sqrt(2.0)
    with np.errstate(all="ignore"):
        for o1, o2, ac, af in FACETS:
            ok = valid & nbv[o1] & nbv[o2]
            e1, e2 = nb[o1], nb[o2]
            s1 = (z64 - e1) / px
            s2 = (e1 - e2) / px
            m0 = s2 < 0
            m1 = ~m0 & (s2 > s1)
            s = np.where(m0, s1, np.where(m1, (z64 - e2) / pxd, np.sqrt(s1 * s1 + s2 * s2)))
            r = np.where(m0, 0.0, np.where(m1, PI / 4, np.arctan2(s2, s1)))
            win = ok & (s > best)
            best = np.where(win, s, best)
            ang = np.where(win, af * r + ac * (PI / 2), ang)
            won |= win
    ang = np.where(ang >= 2 * PI, ang - 2 * PI, ang)
    a32 = ang.astype(np.float32)
    a32[a32 >= F2PI] = 0
    angle = np.where(won, a32, np.float32(-1)).astype(np.float32)
    slope = np.where(won, best.astype(np.float32), np.float32(0)).astype(np.float32)
    if fdr is not None:
        f = np.asarray(fdr)
        for k, code in enumerate(OCT_CODE):
            m = valid & ~won & (f == code) & nbv[k]
            angle[m] = octant_angle(k)
    angle[nod] = -100
    slope[nod] = -100
    return angle, slope


def decode(angle):
    """-> (kind, k, p2) per cell: kind 0 no receiver (-1 / -100), 1 one receiver (octant k), 2 two (octant k with share
    2^30 - p2, octant k + 1 with share p2); ValueError for an angle outside the contract"""
    a = np.asarray(angle, np.float32)
    none = (a == np.float32(-1)) | (a == np.float32(-100))
    ok = none | ((a >= 0) & (a <= F2PI))
    if not ok.all():
        raise ValueError("bad angle")
    t = np.where(none, 0.0, a.astype(np.float64) * FOUR_OVER_PI)
    rt = np.rint(t)
    single = np.abs(t - rt) <= SNAP
    fl = np.floor(t)
    k = np.where(single, rt, fl).astype(np.int64) % 8
    p2 = np.where(single, 0, np.rint((t - fl) * float(ONE))).astype(np.int64)
    kind = np.where(none, 0, np.where(single, 1, 2)).astype(np.int8)
    return kind, k, p2


def receivers(angle):
    """-> (r0, r1, p2): flat index of the receiver at octant k / k + 1 where that edge exists (the receiver lies in
    the raster and is not nodata), -1 elsewhere; plus gone0 / gone1: a share points there but no edge exists"""
    a = np.asarray(angle, np.float32)
    H, W = a.shape
    kind, k, p2 = decode(a)
    nod = a == np.float32(-100)
    yy, xx = np.mgrid[0:H, 0:W]
    dy, dx = np.asarray(OCT_DY), np.asarray(OCT_DX)

    def one(kk, has):
        ny, nx = yy + dy[kk], xx + dx[kk]
        inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        nyc, nxc = np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)
        edge = has & inside & ~nod[nyc, nxc]
        return np.where(edge, nyc * W + nxc, -1).reshape(-1), (has & ~edge).reshape(-1)

    r0, gone0 = one(k, kind >= 1)
    r1, gone1 = one((k + 1) % 8, kind == 2)
    return r0, r1, p2.reshape(-1), gone0, gone1


def share(T, p2):
    """floor(T * p2 / 2^30) for int64 arrays, T < 2^53, p2 <= 2^30: the 83-bit product taken exactly through 26-bit
    halves of T"""
    th, tl = T >> 26, T & ((1 << 26) - 1)
    a = th * p2               # < 2^57
    b = tl * p2               # < 2^56
    return (a + (b >> 26)) >> 4


def quantise(weights, shape, frac_bits):
    if weights is None:
        w = np.ones(shape, np.float64)
    else:
        w = np.asarray(weights, np.float64)
    return np.rint(np.ldexp(w, frac_bits)).astype(np.int64).reshape(-1)


def default_frac_bits(n, wmax):
    if wmax == 0:
        return 0
    return 51 - (n - 1).bit_length() - (math.frexp(wmax)[1] - 1)


def accumulate(angle, weights=None, frac_bits=None, full=False):
    """-> float64 raster; full=True: (result, dict(T, q, done, left, r0, r1)) for the reference's own property tests"""
    a = np.asarray(angle, np.float32)
    H, W = a.shape
    n = H * W
    if frac_bits is None:
        wmax = 1.0 if weights is None else (float(np.max(weights)) if n else 0.0)
        frac_bits = default_frac_bits(n, wmax) if n else 0
    q = quantise(weights, a.shape, frac_bits)
    r0, r1, p2, gone0, gone1 = receivers(a)
    pending = np.bincount(r0[r0 >= 0], minlength=n) + np.bincount(r1[r1 >= 0], minlength=n)
    T = q.copy()
    done = np.zeros(n, bool)
    left = 0
    nod = (a == np.float32(-100)).reshape(-1)
    front = np.flatnonzero((pending == 0) & ~nod)
    while front.size:  # Kahn levels
        done[front] = True
        t = T[front]
        m2 = share(t, p2[front])
        m1 = t - m2
        f0, f1 = r0[front], r1[front]
        e0, e1 = f0 >= 0, f1 >= 0
        np.add.at(T, f0[e0], m1[e0])
        np.add.at(T, f1[e1], m2[e1])
        has_edge = e0 | e1
        left += int(m1[gone0[front] & has_edge].sum()) + int(m2[gone1[front] & has_edge].sum())
        cand = np.concatenate((f0[e0], f1[e1]))
        np.subtract.at(pending, cand, 1)
        cand = cand[pending[cand] == 0]
        front = np.unique(cand)
    res = np.where(done, np.ldexp((T - q).astype(np.float64), -frac_bits), -100.0).reshape(H, W)
    if full:
        return res, dict(T=T, q=q, done=done, left=left, r0=r0, r1=r1, nodata=nod)
    return res
