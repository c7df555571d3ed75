"""The reference of vector.polygonize, numpy and pure Python, written from the definition in descriptools_amd/vector.py
and not from the kernels.  It looks at the lattice VERTEX by vertex: the directed edges of a label that leave a vertex
are found among the four cells around it, a ring is traced edge by edge through `leaving`, and `shell` comes from a
4-connected labelling of equal values -- not from the west walk (tests/test_polygonize_host.py restates that in numpy
and holds the two against each other).  Labels are passed as a plain integer array, so the reference imports nothing of
the package."""
from collections import deque

import numpy as np

E, S, W, N = 0, 1, 2, 3
STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))          # (dy, dx) of a direction
LEFT = ((-1, 0), (0, 1), (1, 0), (0, -1))          # from an edge's own cell to the cell across it
OWNER = ((0, 0), (0, -1), (-1, -1), (-1, 0))       # from a vertex (y, x) to the cell whose edge leaves it in direction d
TAIL = ((0, 0), (0, 1), (1, 1), (1, 0))            # from a cell (i, j) to the tail vertex of its edge d


def normalise(labels, background=None):
    """int64 labels with -1 on background"""
    a = np.asarray(labels)
    out = a.astype(np.int64)
    out[out < 0] = -1
    if background is not None:
        out[a == background] = -1
    return out


def _padded(lab):
    H, Wd = lab.shape
    p = np.full((H + 2, Wd + 2), -1, np.int64)
    p[1:-1, 1:-1] = np.where(lab < 0, -1, lab)
    return p


def _has_edge(p, i, j, d):
    """cell (i, j) carries a directed edge in direction d: it is not background and the cell across differs"""
    L = p[i + 1, j + 1]
    return L >= 0 and p[i + 1 + LEFT[d][0], j + 1 + LEFT[d][1]] != L


def leaving(p, y, x, L):
    """{direction: cell} of the directed edges of label L that leave vertex (y, x)"""
    out = {}
    for d in range(4):
        i, j = y + OWNER[d][0], x + OWNER[d][1]
        if p[i + 1, j + 1] == L and _has_edge(p, i, j, d):
            out[d] = (i, j)
    return out


def components(lab):
    """4-connected components of equal non-negative values: int64 raster of component numbers, -1 on background"""
    H, Wd = lab.shape
    comp = np.full((H, Wd), -1, np.int64)
    n = 0
    flat = lab.tolist()
    for i0 in range(H):
        for j0 in range(Wd):
            L = flat[i0][j0]
            if L < 0 or comp[i0, j0] >= 0:
                continue
            comp[i0, j0] = n
            todo = deque([(i0, j0)])
            while todo:
                i, j = todo.popleft()
                for di, dj in STEP:
                    a, b = i + di, j + dj
                    if 0 <= a < H and 0 <= b < Wd and flat[a][b] == L and comp[a, b] < 0:
                        comp[a, b] = n
                        todo.append((a, b))
            n += 1
    return comp


def shoelace(ring):
    x, y = ring[:, 0], ring[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def polygonize(labels):
    """labels (negative = background) -> (coords float64[N, 2], parts int64[P + 1], ids int32[P], shell int32[P], info)"""
    lab = normalise(labels)
    H, Wd = lab.shape
    p = _padded(lab)
    comp = components(lab)
    edges = []
    for d in range(4):      # _has_edge on the whole raster at once
        across = p[1 + LEFT[d][0]:H + 1 + LEFT[d][0], 1 + LEFT[d][1]:Wd + 1 + LEFT[d][1]]
        edges += [(i, j, d) for i, j in np.argwhere((lab >= 0) & (across != lab)).tolist()]
    index = {e: k for k, e in enumerate(edges)}
    succ = np.zeros(len(edges), np.int64)
    for k, (i, j, d) in enumerate(edges):
        L = p[i + 1, j + 1]
        hy, hx = i + TAIL[d][0] + STEP[d][0], j + TAIL[d][1] + STEP[d][1]
        out = leaving(p, hy, hx, L)
        assert out and (d + 2) & 3 not in out   # straight back is the edge of the cell across, which is not L
        if len(out) == 2:                       # L's cells meet only diagonally here: right and left, and right wins
            assert set(out) == {(d + 1) & 3, (d + 3) & 3}
        nd = next(q for q in ((d + 1) & 3, d, (d + 3) & 3) if q in out)
        succ[k] = index[out[nd] + (nd,)]
    assert sorted(succ.tolist()) == list(range(len(edges))), "the successor is a permutation"
    rings = []
    seen = np.zeros(len(edges), bool)
    for k0 in range(len(edges)):
        if seen[k0]:
            continue
        cycle, k = [], k0
        while not seen[k]:
            seen[k] = True
            cycle.append(k)
            k = int(succ[k])
        assert k == k0
        verts = []
        for a, b in zip(cycle, cycle[1:] + cycle[:1]):
            (i, j, d), nd = edges[a], edges[b][2]
            if nd != d:
                verts.append((i + TAIL[d][0] + STEP[d][0], j + TAIL[d][1] + STEP[d][1]))     # (y, x) of the head
        start = min(verts)
        assert verts.count(start) == 1, "a ring passes its smallest vertex once"
        at = verts.index(start)
        verts = verts[at:] + verts[:at]
        hole = verts[1][0] != verts[0][0]       # leaves southward
        i, j, _ = edges[cycle[0]]
        rings.append((start[0] * (Wd + 1) + start[1], int(hole), verts, int(lab[i, j]), int(comp[i, j])))
    rings.sort(key=lambda r: r[:2])
    order = [r[:2] for r in rings]
    assert len(set(order)) == len(order), "at most one shell and one hole start at a vertex"
    shell_of = {}
    for pos, r in enumerate(rings):
        if not r[1]:
            assert r[4] not in shell_of, "two shells in one 4-connected region"
            shell_of[r[4]] = pos
    assert len(shell_of) == int(comp.max()) + 1, "every 4-connected region has a shell"
    coords = np.array([(x, y) for r in rings for y, x in r[2]], np.float64).reshape(-1, 2)
    parts = np.cumsum([0] + [len(r[2]) for r in rings]).astype(np.int64)
    ids = np.array([r[3] for r in rings], np.int32)
    shell = np.array([shell_of[r[4]] for r in rings], np.int32)
    key = np.array([2 * ((i + TAIL[d][0]) * (Wd + 1) + j + TAIL[d][1]) + (d != E) for i, j, d in edges], np.int64)
    info = {"edges": len(edges), "vertices": int(parts[-1]), "rings": len(rings),
            "holes": sum(r[1] for r in rings), "rounds": doubling_rounds(key, succ)}
    return coords, parts, ids, shell, info


def doubling_rounds(key, succ):
    """Round k >= 1 replaces every window's smallest key m by min(m, m[jump]) and the jump by its square; the number of
    the first round that lowers nothing"""
    m, jump, rounds = key.copy(), succ.copy(), 0
    while True:
        rounds += 1
        lower = np.minimum(m, m[jump])
        if (lower == m).all():
            return rounds
        m, jump = lower, jump[jump]
