"""The numpy / Python reference of descriptools_amd.cost (its module docstring holds the definition): a heap Dijkstra
in float64 with the definition's association, the back-link scan, the roots of the back-link trees, a randomly ordered
tile relaxation that pins the uniqueness claim, and the rasters the host and the GPU tests share."""
import heapq

import numpy as np

SQRT2 = 1.4142135623730951
# the scan order of the back-link: NW, N, NE, W, E, SW, S, SE -> (dy, dx, ESRI code)
SCAN = ((-1, -1, 32), (-1, 0, 64), (-1, 1, 128), (0, -1, 16), (0, 1, 1), (1, -1, 8), (1, 0, 4), (1, 1, 2))


def passable(friction):
    f = np.asarray(friction, np.float32)
    with np.errstate(invalid="ignore"):
        return (f > 0) & (f < np.inf)


def _moves(connectivity):
    return [m for m in SCAN if connectivity == 8 or m[0] == 0 or m[1] == 0]


def _edge(px, dy, dx, fu, fv):
    """w(u, v) on Python floats: IEEE float64, one rounding per operation (an overflow gives +inf)"""
    step = px * SQRT2 if dy and dx else px
    return step * ((fu + fv) * 0.5)


def _setup(friction, sources, px):
    """(friction as lists of Python floats, passable and source masks as lists, H, W, px as a Python float)"""
    f = np.asarray(friction, np.float32)
    ok = passable(f)
    src = ok & (np.asarray(sources).astype(np.int8) == 1)
    return f.astype(np.float64).tolist(), ok.tolist(), src.tolist(), f.shape[0], f.shape[1], float(px)


def dijkstra(friction, sources, px, connectivity=8):
    """A (float64, +inf on barriers and unreached cells) by a heap Dijkstra"""
    f, ok, src, H, W, px = _setup(friction, sources, px)
    inf = float("inf")
    A = [[0.0 if src[y][x] else inf for x in range(W)] for y in range(H)]
    heap = [(0.0, y, x) for y in range(H) for x in range(W) if src[y][x]]
    heapq.heapify(heap)
    moves = _moves(connectivity)
    while heap:
        a, y, x = heapq.heappop(heap)
        if a > A[y][x]:
            continue
        for dy, dx, _ in moves:
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and ok[ny][nx]:
                c = a + _edge(px, dy, dx, f[y][x], f[ny][nx])
                if c < A[ny][nx]:
                    A[ny][nx] = c
                    heapq.heappush(heap, (c, ny, nx))
    return np.array(A, np.float64).reshape(H, W)


def tile_relaxation(friction, sources, px, connectivity, tile, seed):
    """A by relaxing tiles of `tile` x `tile` cells in a random order, the cells of a tile in a random order, from
    +inf, until a pass over all tiles lowers nothing"""
    f, ok, src, H, W, px = _setup(friction, sources, px)
    inf = float("inf")
    A = [[0.0 if src[y][x] else inf for x in range(W)] for y in range(H)]
    moves = _moves(connectivity)
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
                    for dy, dx, _ in moves:
                        ny, nx = y + dy, x + dx
                        if 0 <= ny < H and 0 <= nx < W and ok[ny][nx] and A[ny][nx] < inf:
                            c = A[ny][nx] + _edge(px, dy, dx, f[ny][nx], f[y][x])
                            if c < A[y][x]:
                                A[y][x] = c
                                again = changed = True
    return np.array(A, np.float64).reshape(H, W)


def backlinks(friction, sources, px, connectivity, A):
    """(backlink uint8, parent int64 flat index or -1, the number of reached non-source cells without a link)"""
    f, ok, src, H, W, px = _setup(friction, sources, px)
    inf = float("inf")
    A = np.asarray(A, np.float64).tolist()
    link = np.zeros((H, W), np.uint8)
    parent = np.full((H, W), -1, np.int64)
    moves = _moves(connectivity)
    linkless = 0
    for y in range(H):
        for x in range(W):
            if not ok[y][x] or not A[y][x] < inf:
                continue
            if src[y][x]:
                parent[y, x] = y * W + x
                continue
            for dy, dx, code in moves:
                ny, nx = y + dy, x + dx
                if 0 <= ny < H and 0 <= nx < W and ok[ny][nx] and A[ny][nx] < A[y][x] and \
                        A[ny][nx] + _edge(px, dy, dx, f[ny][nx], f[y][x]) == A[y][x]:
                    link[y, x] = code
                    parent[y, x] = ny * W + nx
                    break
            else:
                linkless += 1
    return link, parent, linkless


def roots(parent):
    """the root of every cell's parent chain (-1 where the chain has none)"""
    p = parent.reshape(-1).copy()
    idx = np.arange(p.size)
    p = np.where(p < 0, -1, p)
    while True:
        up = np.where(p >= 0, p, idx)
        q = np.where(p >= 0, p[up], -1)
        if np.array_equal(q, p):
            return p.reshape(parent.shape)
        p = q


def reference(friction, sources, px, connectivity=8):
    """(cost float64, indices int64, backlink uint8, linkless count, reached count) with the -100 / -100 / 0 fills"""
    A = dijkstra(friction, sources, px, connectivity)
    link, parent, linkless = backlinks(friction, sources, px, connectivity, A)
    root = roots(parent)
    reached = passable(friction) & (A < np.inf)
    cost = np.where(reached, A, -100.0)
    indices = np.where(root >= 0, root, -100).astype(np.int64)
    return cost, indices, link, linkless, int(reached.sum())


# ---- the rasters the tests share -----------------------------------------------------------------------------------
KINDS = ("uniform", "integer", "exp")


def random_case(shape, kind, seed):
    """(friction float32 with 25 % barriers, sources int8 at about 0.4 % of the cells)"""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        f = rng.uniform(0.5, 2.0, shape).astype(np.float32)
    elif kind == "integer":
        f = rng.integers(1, 4, shape).astype(np.float32)
    else:
        f = np.exp(rng.uniform(-20, 20, shape)).astype(np.float32)
    bar = rng.random(shape) < 0.25
    # every kind of barrier the definition names
    f[bar] = rng.choice(np.array([0, -1, -100, np.nan, np.inf], np.float32), int(bar.sum()))
    s = (rng.random(shape) < 0.004).astype(np.int8)
    return f, s


def serpentine(shape=(130, 257)):
    """friction 1, a barrier column at every x = 3, 7, 11, ... with one gap, alternately at the bottom and at the top,
    one source at (0, 0)"""
    H, W = shape
    f = np.ones(shape, np.float32)
    for i, x in enumerate(range(3, W, 4)):
        f[:, x] = 0
        f[H - 1 if i % 2 == 0 else 0, x] = 1
    s = np.zeros(shape, np.int8)
    s[0, 0] = 1
    return f, s


def path_tile_entries(parent, start, tile):
    """(cells on the back-link path from flat index `start` to its root, the number of times the path enters a tile)"""
    W = parent.shape[1]
    p = parent.reshape(-1)
    c, cells, entries, last = int(start), 0, 0, None
    while True:
        cells += 1
        t = (c // W // tile, c % W // tile)
        if t != last:
            entries += 1
            last = t
        if p[c] == c or p[c] < 0:
            return cells, entries
        c = int(p[c])
