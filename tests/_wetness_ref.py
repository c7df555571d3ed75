"""The numpy / Python reference of descriptools_amd.wetness (its module docstring holds the definition): the suction
and the index in numpy float64 with the definition's association, a max-heap Dijkstra for the modified area, Jacobi
sweeps that return their count, a randomly ordered tile relaxation that pins the uniqueness claim, and the rasters the
host and the GPU tests share."""
import heapq
import math

import numpy as np

SLOPE_OFFSET = math.radians(0.1)
HALF_PI = math.pi / 2
TINY32 = float(np.finfo(np.float32).tiny)
MOVES = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _slope_ok(slope):
    sl = np.asarray(slope, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return sl, (sl >= 0) & (sl < HALF_PI)


def beta(slope, slope_offset=SLOPE_OFFSET, slope_min=0.0):
    """b = max(float64(slope) + slope_offset, slope_min); NaN where the slope is NaN or not in [0, pi/2)"""
    sl, ok = _slope_ok(slope)
    return np.where(ok, np.maximum(np.where(ok, sl, 0.0) + slope_offset, slope_min), np.nan)


def suction(slope, t=10.0, slope_weight=1.0, slope_offset=SLOPE_OFFSET, slope_min=0.0):
    """float32, -100 where the slope is NaN or not in [0, pi/2); one rounding per operation"""
    b = beta(slope, slope_offset, slope_min)
    ok = ~np.isnan(b)
    e = slope_weight * np.where(ok, b, 0.0)
    L = math.log(t)
    with np.errstate(over="ignore", under="ignore"):
        s = np.exp(-((e * np.exp(np.exp(e * L))) * L))
    s = np.where(s < TINY32, 0.0, s)
    return np.where(ok, s, -100.0).astype(np.float32)


def valid(area, suct):
    a = np.asarray(area, np.float64)
    s = np.asarray(suct, np.float32)
    with np.errstate(invalid="ignore"):
        return (a > 0) & (a < np.inf) & (s >= 0) & (s <= 1)


def swi(modified, slope, slope_offset=SLOPE_OFFSET, slope_min=0.0):
    """float32(log(M / tan(b))), -100 where M is not in (0, +inf), the slope is out of range or b >= pi/2"""
    m = np.asarray(modified, np.float64)
    b = beta(slope, slope_offset, slope_min)
    with np.errstate(invalid="ignore"):
        ok = (m > 0) & (m < np.inf) & (b < HALF_PI)
    with np.errstate(all="ignore"):
        v = np.log(np.where(ok, m, 1.0) / np.tan(np.where(ok, b, 1.0)))
    return np.where(ok, v, -100.0).astype(np.float32)


def _setup(area, suct):
    """(area and suction as lists of Python floats, the valid mask as lists, H, W)"""
    a = np.asarray(area, np.float64)
    s = np.asarray(suct, np.float32)
    ok = valid(a, s)
    return a.tolist(), s.astype(np.float64).tolist(), ok.tolist(), a.shape[0], a.shape[1]


def _fill(M, ok, H, W):
    out = np.array(M, np.float64).reshape(H, W)
    out[~np.array(ok, bool).reshape(H, W)] = -100.0
    return out


def dijkstra(area, suct):
    """M (float64, -100 on nodata) by a max-heap Dijkstra: the largest value is final when it is popped, because no
    product exceeds its factor"""
    a, s, ok, H, W = _setup(area, suct)
    M = [[a[y][x] if ok[y][x] else -math.inf for x in range(W)] for y in range(H)]
    heap = [(-M[y][x], y, x) for y in range(H) for x in range(W) if ok[y][x]]
    heapq.heapify(heap)
    while heap:
        m, y, x = heapq.heappop(heap)
        m = -m
        if m < M[y][x]:
            continue
        for dy, dx in MOVES:
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and ok[ny][nx]:
                c = s[ny][nx] * m
                if c > M[ny][nx]:
                    M[ny][nx] = c
                    heapq.heappush(heap, (-c, ny, nx))
    return _fill(M, ok, H, W)


reference = dijkstra


def jacobi(area, suct):
    """(M, the number of sweeps that raised something) by plain Jacobi sweeps in numpy: every cell reads the previous
    sweep's neighbours"""
    a = np.asarray(area, np.float64)
    s = np.asarray(suct, np.float32).astype(np.float64)
    ok = valid(a, s)
    H, W = a.shape
    M = np.where(ok, a, -np.inf)
    s = np.where(ok, s, 0.0)
    sweeps = 0
    while True:
        P = np.full((H + 2, W + 2), -np.inf)
        P[1:-1, 1:-1] = M
        top = np.full((H, W), -np.inf)
        for dy, dx in MOVES:
            top = np.maximum(top, P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        with np.errstate(invalid="ignore"):
            cand = s * top  # 0 * -inf = NaN never compares greater
            up = ok & (cand > M)
        if not up.any():
            return np.where(ok, M, -100.0), sweeps
        M = np.where(up, cand, M)
        sweeps += 1


def tile_relaxation(area, suct, tile, seed):
    """M by relaxing tiles of `tile` x `tile` cells in a random order, the cells of a tile in a random order, from
    M = A, until a pass over all tiles raises nothing"""
    a, s, ok, H, W = _setup(area, suct)
    M = [[a[y][x] if ok[y][x] else -math.inf for x in range(W)] for y in range(H)]
    rng = np.random.default_rng(seed)
    tiles = [(ty, tx) for ty in range(0, H, tile) for tx in range(0, W, tile)]
    changed = True
    while changed:
        changed = False
        for t in rng.permutation(len(tiles)):
            ty, tx = tiles[t]
            cells = [(y, x) for y in range(ty, min(ty + tile, H)) for x in range(tx, min(tx + tile, W)) if ok[y][x]]
            again = True
            while again:
                again = False
                for i in rng.permutation(len(cells)):
                    y, x = cells[i]
                    for dy, dx in MOVES:
                        ny, nx = y + dy, x + dx
                        if 0 <= ny < H and 0 <= nx < W and ok[ny][nx]:
                            c = s[y][x] * M[ny][nx]
                            if c > M[y][x]:
                                M[y][x] = c
                                again = changed = True
    return _fill(M, ok, H, W)


def raised(area, suct, M):
    """the number of valid cells with M > A"""
    ok = valid(area, suct)
    return int((ok & (np.asarray(M) > np.where(ok, np.asarray(area, np.float64), np.inf))).sum())


# ---- the rasters the tests share -----------------------------------------------------------------------------------
KINDS = ("uniform", "plateau", "steep")


def random_case(shape, kind, seed):
    """(area float64 with about 10 % nodata of every kind, suction float32 with about 4 % out of range)"""
    rng = np.random.default_rng(seed)
    a = np.exp(rng.uniform(0, 14, shape))
    if kind == "uniform":
        s = rng.uniform(0.3, 1.0, shape).astype(np.float32)
    elif kind == "plateau":
        s = rng.uniform(0.9, 1.0, shape).astype(np.float32)
        s[rng.random(shape) < 0.3] = 1.0
        a = np.floor(a)  # integers >= 1: exact ties and long fronts
    else:
        s = (rng.random(shape) ** 4).astype(np.float32)
        s[rng.random(shape) < 0.1] = 0.0
    bad = rng.random(shape) < 0.10
    a[bad] = rng.choice(np.array([np.nan, -100.0, np.inf, 0.0, -1.0]), int(bad.sum()))
    bad = rng.random(shape) < 0.04
    s[bad] = rng.choice(np.array([np.nan, np.nextafter(np.float32(1), np.float32(2)),
                                  np.nextafter(np.float32(0), np.float32(-1)), -100.0], np.float32), int(bad.sum()))
    return a, s


def serpentine(shape=(130, 257), s=1.0):
    """area 1, a nodata column at every x = 3, 7, 11, ... with one gap, alternately at the bottom and at the top, area
    1e6 at (0, 0); suction `s` everywhere (tests/_cost_ref.serpentine's layout)"""
    H, W = shape
    a = np.ones(shape, np.float64)
    for i, x in enumerate(range(3, W, 4)):
        a[:, x] = -100.0
        a[H - 1 if i % 2 == 0 else 0, x] = 1.0
    a[0, 0] = 1e6
    return a, np.full(shape, s, np.float32)


def serpentine_tile_entries(shape=(130, 257), tile=64):
    """the number of times the path from (0, 0) through the gaps to the last column enters a tile of `tile` cells"""
    H, W = shape
    entries, last = 0, None
    bars = list(range(3, W, 4))
    x0 = 0
    for i in range(len(bars) + 1):
        x1 = bars[i] if i < len(bars) else W  # the corridor x0 .. x1 - 1, walked down (even i) or up (odd i)
        rows = range(H) if i % 2 == 0 else range(H - 1, -1, -1)
        for y in rows:
            t = (y // tile, x0 // tile)
            if t != last:
                entries, last = entries + 1, t
        if i < len(bars):
            y = H - 1 if i % 2 == 0 else 0
            for x in range(x0, x1 + 1):  # along the gap's row into the next corridor
                t = (y // tile, x // tile)
                if t != last:
                    entries, last = entries + 1, t
        x0 = x1 + 1
    return entries
