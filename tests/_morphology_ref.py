"""The references of descriptools_amd.morphology, in plain Python and numpy: the order-preserving key and its inverse,
the max-heap Dijkstra (widest path) on keys with erosion by complement, an independent Jacobi iteration, a brute-force
plateau labelling for the regional extrema, a sequential priority flood for the fill, and the rasters the tests share.
The module docstring of descriptools_amd/morphology.py holds the definitions; nothing here calls the library."""
import heapq
from collections import deque

import numpy as np

NB8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
NB4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
ALL = np.uint32(0xFFFFFFFF)
# the float32 next above -100: the floor of the h-maxima marker
FLOOR = np.nextafter(np.float32(-100), np.float32(np.inf))


def key(a):
    """the order-preserving uint32 key of float32 bits: a < b as floats <=> key(a) < key(b); -0.0 below +0.0"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(u >> 31 == 0, u ^ np.uint32(0x80000000), ~u).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def valid(z):
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > -100)


def given(m):
    """where a user marker is given: not NaN and > -100 (+inf is given)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(m, np.float32) > -100


def _nb(cn):
    return NB8 if cn == 8 else NB4


def start_keys(marker, mask, erosion, is_given=None):
    """(F0, G, ok) on the keys the dilation runs on (complemented for erosion): G the clamp key, 0 on invalid cells;
    F0 = min(marker key, G) where the marker is given (`is_given`: a bool raster, default the user-marker rule), 0 = none
    elsewhere"""
    mask = np.asarray(mask, np.float32)
    marker = np.asarray(marker, np.float32)
    ok = valid(mask)
    flip = ALL if erosion else np.uint32(0)
    G = np.where(ok, key(mask) ^ flip, 0).astype(np.uint32)
    giv = given(marker) if is_given is None else np.asarray(is_given, bool)
    F = np.where(ok & giv, np.minimum(key(marker) ^ flip, G), 0).astype(np.uint32)
    return F, G, ok


def dijkstra_keys(F, G, cn=8):
    """the reconstruction by dilation on keys: the widest path, by a max-heap"""
    H, W = G.shape
    g = [int(v) for v in G.ravel()]
    r = [int(v) for v in F.ravel()]
    heap = [(-v, i) for i, v in enumerate(r) if v]
    heapq.heapify(heap)
    nb = _nb(cn)
    while heap:
        v, i = heapq.heappop(heap)
        v = -v
        if v != r[i]:
            continue
        y, x = divmod(i, W)
        for dy, dx in nb:
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W:
                j = ny * W + nx
                c = v if v < g[j] else g[j]
                if c > r[j]:
                    r[j] = c
                    heapq.heappush(heap, (-c, j))
    return np.asarray(r, np.uint32).reshape(H, W)


def jacobi_keys(F, G, cn=8):
    """(R, sweeps that changed something) by plain Jacobi sweeps in numpy"""
    R = F.copy()
    H, W = R.shape
    sweeps = 0
    while True:
        P = np.pad(R, 1)
        m = R.copy()
        for dy, dx in _nb(cn):
            m = np.maximum(m, P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        N = np.minimum(m, G)
        if np.array_equal(N, R):
            return R, sweeps
        R = N
        sweeps += 1


def from_keys(R, erosion):
    """keys of the dilation back to float32: -100 for none"""
    flip = ALL if erosion else np.uint32(0)
    return np.where(R == 0, np.float32(-100), unkey(R ^ flip)).astype(np.float32)


def reconstruct(marker, mask, kind="dilation", cn=8, is_given=None):
    e = kind == "erosion"
    F, G, _ = start_keys(marker, mask, e, is_given)
    return from_keys(dijkstra_keys(F, G, cn), e)


def jacobi(marker, mask, kind="dilation", cn=8, is_given=None):
    e = kind == "erosion"
    F, G, _ = start_keys(marker, mask, e, is_given)
    R, sweeps = jacobi_keys(F, G, cn)
    return from_keys(R, e), sweeps


def changed(marker, mask, kind, R, is_given=None):
    """the number of valid cells whose result is not their start value"""
    e = kind == "erosion"
    F, _, ok = start_keys(marker, mask, e, is_given)
    return int((ok & (from_keys(F, e).view(np.uint32) != np.asarray(R, np.float32).view(np.uint32))).sum())


# ---- the derived markers ---------------------------------------------------------------------------------------------
def default_outlets(dem):
    """valid cells on the raster's edge or with an invalid 8-neighbour"""
    ok = valid(dem)
    H, W = ok.shape
    P = np.pad(ok, 1, constant_values=True)
    bad = np.zeros(ok.shape, bool)
    for dy, dx in NB8:
        bad |= ~P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    edge = np.zeros(ok.shape, bool)
    if ok.size:
        edge[0] = edge[-1] = True
        edge[:, 0] = edge[:, -1] = True
    return ok & (edge | bad)


def fill(dem, outlets=None, cn=8):
    dem = np.asarray(dem, np.float32)
    out = default_outlets(dem) if outlets is None else (np.asarray(outlets) != 0)
    return reconstruct(dem, dem, "erosion", cn, is_given=out)


def priority_flood(dem, outlets=None, cn=8):
    """the fill by a sequential priority flood on float heights (ties by key, so -0.0 / +0.0 come out as the key order
    selects); -100 on invalid cells and on cells that reach no outlet"""
    dem = np.asarray(dem, np.float32)
    ok = valid(dem)
    H, W = dem.shape
    out = (default_outlets(dem) if outlets is None else (np.asarray(outlets) != 0)) & ok
    k = key(dem)
    res = np.zeros(dem.shape, np.uint32)
    done = out.copy()
    heap = [(int(k[y, x]), y, x) for y, x in zip(*np.nonzero(out))]
    for v, y, x in heap:
        res[y, x] = v
    heapq.heapify(heap)
    while heap:
        w, y, x = heapq.heappop(heap)
        for dy, dx in _nb(cn):
            v, u = y + dy, x + dx
            if 0 <= v < H and 0 <= u < W and ok[v, u] and not done[v, u]:
                done[v, u] = True
                res[v, u] = max(w, int(k[v, u]))
                heapq.heappush(heap, (int(res[v, u]), v, u))
    return np.where(done, unkey(res), np.float32(-100)).astype(np.float32)


def h_marker(dem, h, maxima):
    """the stated float64 marker of hminima / hmaxima, given on every valid cell"""
    z = np.asarray(dem, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if maxima:
            return np.maximum((z - h).astype(np.float32), FLOOR)
        return (z + h).astype(np.float32)


def h_extrema(dem, h, maxima, cn=8):
    dem = np.asarray(dem, np.float32)
    return reconstruct(h_marker(dem, h, maxima), dem, "dilation" if maxima else "erosion", cn, is_given=valid(dem))


def regional(dem, maxima, cn=8):
    """uint8: 1 on the plateaus (connected cells of one key) with no strictly lower (higher) valid neighbour, by
    labelling every plateau"""
    dem = np.asarray(dem, np.float32)
    ok = valid(dem)
    k = key(dem).astype(np.int64)
    if maxima:
        k = -k
    H, W = dem.shape
    seen = np.zeros(dem.shape, bool)
    out = np.zeros(dem.shape, np.uint8)
    nb = _nb(cn)
    for y in range(H):
        for x in range(W):
            if not ok[y, x] or seen[y, x]:
                continue
            comp = [(y, x)]
            seen[y, x] = True
            q = deque(comp)
            extreme = True
            while q:
                a, b = q.popleft()
                for dy, dx in nb:
                    v, u = a + dy, b + dx
                    if 0 <= v < H and 0 <= u < W and ok[v, u]:
                        if k[v, u] == k[a, b]:
                            if not seen[v, u]:
                                seen[v, u] = True
                                q.append((v, u))
                                comp.append((v, u))
                        elif k[v, u] < k[a, b]:
                            extreme = False
            if extreme:
                for a, b in comp:
                    out[a, b] = 1
    return out


def regional_by_reconstruction(dem, maxima, cn=8):
    """the same through the definition: R != mask with the marker key = mask key + 1 (erosion) or - 1 (dilation)"""
    dem = np.asarray(dem, np.float32)
    ok = valid(dem)
    flip = np.uint32(0) if maxima else ALL
    G = np.where(ok, key(dem) ^ flip, 0).astype(np.uint32)
    F = np.where(ok, G - np.uint32(1), 0).astype(np.uint32)
    return (ok & (dijkstra_keys(F, G, cn) != G)).astype(np.uint8)


# ---- the rasters the tests share -----------------------------------------------------------------------------------
FIELDS = ("uniform", "rounded", "nodata")


def random_case(shape, field, seed):
    """(marker, mask) float32.  uniform: random heights; rounded: heights rounded to 0.5 m (plateaus, exact ties);
    nodata: rounded, with blobs of every kind of invalid cell in the mask (-100, below it, NaN, +inf, -inf) and of NaN,
    +inf and <= -100 in the marker.  The marker lies within 10 m of the mask, above or below"""
    rng = np.random.default_rng(seed)
    H, W = shape
    z = rng.uniform(3.0, 53.0, shape)
    if field != "uniform":
        z = np.round(z * 2) / 2
    mask = z.astype(np.float32)
    marker = (z + rng.uniform(-10.0, 10.0, shape)).astype(np.float32)
    if field == "nodata":
        def blobs(a, values, n):
            for i in range(n):
                y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
                h, w = int(rng.integers(1, 7)), int(rng.integers(1, 7))
                a[y:y + h, x:x + w] = values[i % len(values)]
        n = max(5, H * W // 400)
        blobs(mask, [-100.0, -9999.0, np.nan, np.inf, -np.inf], n)
        blobs(marker, [np.inf, np.nan, -100.0, -np.inf, np.inf], n)
    return marker, mask


def dem_with_voids(shape, seed):
    """heights rounded to 0.5 m with blobs of -100 and below: the DEM of the fill tests"""
    rng = np.random.default_rng(seed)
    H, W = shape
    z = (np.round(rng.uniform(3.0, 53.0, shape) * 2) / 2).astype(np.float32)
    for i in range(max(3, H * W // 3000)):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        z[y:y + int(rng.integers(1, 9)), x:x + int(rng.integers(1, 9))] = (-100.0, -9999.0)[i % 2]
    return z


def serpentine(n=192, high=10.0, low=1.0):
    """(marker, mask): corridors of height `high` on the even rows between walls of height `low` on the odd rows, each
    wall with one gap, alternately at the right and at the left end: one path of n / 2 rows that winds through every
    tile.  The marker sits at (0, 0) only (NaN elsewhere)"""
    mask = np.full((n, n), high, np.float32)
    for i, y in enumerate(range(1, n, 2)):
        mask[y, :] = low
        mask[y, n - 1 if i % 2 == 0 else 0] = high
    marker = np.full((n, n), np.nan, np.float32)
    marker[0, 0] = high
    return marker, mask


def spiral(n=64, high=10.0, low=1.0):
    """(marker, mask): a one-cell corridor that spirals inwards from (0, 0) between one-cell walls; the marker sits at
    (0, 0) only"""
    c = np.zeros((n, n), bool)
    y = x = 0
    c[0, 0] = True
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    d = turns = 0
    inside = lambda a, b: 0 <= a < n and 0 <= b < n
    while turns < 2:
        dy, dx = dirs[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(y1, x1) and not c[y1, x1] and (not inside(y2, x2) or not c[y2, x2]):
            y, x = y1, x1
            c[y, x] = True
            turns = 0
        else:
            d = (d + 1) % 4
            turns += 1
    mask = np.where(c, np.float32(high), np.float32(low)).astype(np.float32)
    marker = np.full((n, n), np.nan, np.float32)
    marker[0, 0] = high
    return marker, mask
