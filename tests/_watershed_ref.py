"""Pure-numpy reference of descriptools_amd.watershed, independent of the kernels: drainage and watersheds by vectorised
pointer doubling on (ptr, n_card, n_diag), upslope_length by in-degree peeling with the exact pair comparison.

Shared by tests/test_watershed_host.py (which checks it on hand-built cases) and tests/test_gpu_watershed.py (which
holds the GPU to it cell for cell)."""
import numpy as np

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
DY = {E: 0, SE: 1, S: 1, SW: 1, W_: 0, NW: -1, N: -1, NE: -1}
DX = {E: 1, SE: 1, S: 0, SW: -1, W_: -1, NW: -1, N: 0, NE: 1}
DIAG = (SE, SW, NW, NE)


def graph(fdr, dem=None):
    """(valid, succ, diag): valid = not nodata; succ[c] = flat index of c's successor, -1 at terminals and nodata;
    diag[c] = the edge is a diagonal move"""
    fdr = np.asarray(fdr, np.uint8)
    H, W = fdr.shape
    n = H * W
    valid = np.ones(n, bool) if dem is None else ~(np.asarray(dem) <= -100).reshape(-1)
    f = fdr.reshape(-1)
    succ = np.full(n, -1, np.int64)
    diag = np.zeros(n, bool)
    y, x = np.divmod(np.arange(n, dtype=np.int64), max(W, 1))
    for code in DY:
        m = (f == code) & valid
        ty, tx = y[m] + DY[code], x[m] + DX[code]
        ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        idx = np.flatnonzero(m)[ok]
        t = ty[ok] * W + tx[ok]
        keep = valid[t]
        succ[idx[keep]] = t[keep]
        diag[idx[keep]] = code in DIAG
    return valid, succ, diag


def length(card, diag, px):
    return card.astype(np.float64) * px + diag.astype(np.float64) * (px * np.sqrt(2.0))


def drainage(fdr, px=1.0, dem=None, pour_points=None):
    """(target int64, length float64, label int64 or None) by the definition in descriptools_amd/watershed.py"""
    fdr = np.asarray(fdr, np.uint8)
    H, W = fdr.shape
    n = H * W
    valid, succ, dg = graph(fdr, dem)
    pour = None if pour_points is None else np.asarray(pour_points, np.int64).reshape(-1)
    stop = valid & (succ < 0) if pour is None else valid & (pour > 0)
    bad = valid & (succ < 0) & ~stop            # a terminal that is no pour point: the path ends there, no target
    end = stop | bad | ~valid
    ptr = np.where(end, np.arange(n, dtype=np.int64), succ)
    card = np.where(end, 0, ~dg).astype(np.int64)
    diag = np.where(end, 0, dg).astype(np.int64)
    rounds = 1
    while (1 << (rounds - 1)) < max(n, 1):
        rounds += 1
    for _ in range(rounds + 1):
        open_ = ~end[ptr]
        if not open_.any():
            break
        nxt = ptr[ptr]
        card = card + card[ptr]
        diag = diag + diag[ptr]
        ptr = nxt
        card = np.minimum(card, 1 << 40)        # on a cycle only; keeps the sums bounded
        diag = np.minimum(diag, 1 << 40)
    good = valid & stop[ptr]
    target = np.where(good, ptr, -100).astype(np.int64)
    ln = np.where(good, length(card, diag, px), -100.0)
    label = None
    if pour is not None:
        label = np.where(good, pour[np.where(good, ptr, 0)], np.where(valid & bad[ptr], 0, -100)).astype(np.int64)
        label = label.reshape(H, W)
    return target.reshape(H, W), ln.reshape(H, W), label


def pair_greater(a1, b1, a2, b2):
    """a1 + b1 sqrt(2) > a2 + b2 sqrt(2), exactly (object arithmetic: no overflow)"""
    da = np.asarray(a1, object) - np.asarray(a2, object)
    db = np.asarray(b1, object) - np.asarray(b2, object)
    da2 = da * da
    db2 = 2 * db * db
    pos = ((da >= 0) & (db >= 0) & ~((da == 0) & (db == 0))) | ((da > 0) & (db < 0) & (da2 > db2)) \
        | ((da < 0) & (db > 0) & (db2 > da2))
    return np.asarray(pos).astype(bool)


def upslope_length(fdr, px=1.0, dem=None):
    """float64 upslope length by in-degree peeling; -100 on nodata and on cells of a D8 cycle"""
    fdr = np.asarray(fdr, np.uint8)
    H, W = fdr.shape
    n = H * W
    valid, succ, dg = graph(fdr, dem)
    has = succ >= 0
    indeg = np.bincount(succ[has], minlength=n).astype(np.int64)
    bc = np.zeros(n, np.int64)   # the best pair so far: n_card, n_diag
    bd = np.zeros(n, np.int64)
    done = np.zeros(n, bool)
    front = np.flatnonzero(valid & (indeg == 0))
    while front.size:
        done[front] = True
        f = front[succ[front] >= 0]
        t = succ[f]
        ca = bc[f] + (~dg[f]).astype(np.int64)
        cb = bd[f] + dg[f].astype(np.int64)
        # fold the candidates into their targets, one candidate per target at a time (in-degree <= 8)
        o = np.argsort(t, kind="stable")
        f, t, ca, cb = f[o], t[o], ca[o], cb[o]
        first = np.r_[0, np.flatnonzero(np.diff(t)) + 1] if t.size else np.zeros(0, np.int64)
        rank = np.arange(t.size) - np.repeat(first, np.diff(np.r_[first, t.size]))
        for r in range(int(rank.max()) + 1 if t.size else 0):
            m = rank == r
            tt = t[m]
            g = pair_greater(ca[m], cb[m], bc[tt], bd[tt])
            bc[tt[g]] = ca[m][g]
            bd[tt[g]] = cb[m][g]
        np.subtract.at(indeg, t, 1)
        cand = np.unique(t)
        front = cand[(indeg[cand] == 0) & ~done[cand]]
    out = np.where(valid & done, length(bc, bd, px), -100.0)
    return out.reshape(H, W)


def hand_cases():
    """name -> (fdr, dem or None, pour or None, px, expected target, expected length, expected label or None,
    expected upslope)"""
    r2 = np.sqrt(2.0)
    c = {}
    # one row draining east to an outlet at the east edge (its code points off the raster)
    fdr = np.array([[E, E, E, E]], np.uint8)
    c["row_to_edge"] = (fdr, None, None, 2.0, np.array([[3, 3, 3, 3]]), np.array([[6.0, 4.0, 2.0, 0.0]]), None,
                        np.array([[0.0, 2.0, 4.0, 6.0]]))
    # code 0 and a non-D8 code are terminals
    fdr = np.array([[E, 0, W_, 3]], np.uint8)
    c["code0_and_non_d8"] = (fdr, None, None, 1.0, np.array([[1, 1, 1, 3]]), np.array([[1.0, 0.0, 1.0, 0.0]]),
                             None, np.array([[0.0, 1.0, 0.0, 0.0]]))
    # a diagonal: (0,0) -> SE (1,1) -> E (1,2), which points into nodata (1,3): a terminal
    fdr = np.array([[SE, 0, 0, 0], [0, E, E, E]], np.uint8)
    dem = np.array([[1, 1, 1, 1], [1, 1, 1, -100]], np.float32)
    c["diagonal_into_nodata"] = (fdr, dem, None, 1.0, np.array([[6, 1, 2, 3], [4, 6, 6, -100]]),
                                 np.array([[1.0 + r2, 0, 0, 0], [0, 1.0, 0.0, -100]]), None,
                                 np.array([[0, 0, 0, 0], [0, r2, 1.0 + r2, -100]]))
    # a 2 x 2 cycle with a tributary draining into it
    fdr = np.array([[E, S, 0], [N, W_, W_]], np.uint8)
    c["cycle_with_tributary"] = (fdr, None, None, 1.0, np.array([[-100, -100, 2], [-100, -100, -100]]),
                                 np.array([[-100.0, -100, 0], [-100, -100, -100]]), None,
                                 np.array([[-100.0, -100, 0], [-100, -100, 0]]))
    # pour points: a row with pour points at x = 1 (label 7) and x = 3 (label 9), terminal at x = 4
    fdr = np.array([[E, E, E, E, 0]], np.uint8)
    pour = np.array([[0, 7, 0, 9, 0]], np.int64)
    c["nested_pour_points"] = (fdr, None, pour, 1.0, np.array([[1, 1, 3, 3, -100]]),
                               np.array([[1.0, 0, 1, 0, -100]]), np.array([[7, 7, 9, 9, 0]]),
                               np.array([[0.0, 1, 2, 3, 4]]))
    # a pour point on a cycle stops it; a pour point off every path is never met
    fdr = np.array([[E, S, 0], [N, W_, 0]], np.uint8)
    pour = np.array([[0, 5, 3], [0, 0, 0]], np.int64)
    c["pour_point_on_cycle"] = (fdr, None, pour, 1.0, np.array([[1, 1, 2], [1, 1, -100]]),
                                np.array([[1.0, 0, 0], [2, 3, -100]]), np.array([[5, 5, 3], [5, 5, 0]]),
                                np.array([[-100.0, -100, 0], [-100, -100, 0]]))
    # a pour point on nodata is ignored: the cell above it becomes a terminal without a pour point
    fdr = np.array([[S], [S], [0]], np.uint8)
    dem = np.array([[1], [-200], [1]], np.float32)
    pour = np.array([[0], [4], [2]], np.int64)
    c["pour_point_on_nodata"] = (fdr, dem, pour, 1.0, np.array([[-100], [-100], [2]]),
                                 np.array([[-100.0], [-100], [0]]), np.array([[0], [-100], [2]]),
                                 np.array([[0.0], [-100], [0]]))
    # two branches into (2,3): three cardinal moves (3.0) beat two diagonal ones (2.83)
    fdr = np.array([[0, SE, E, S], [0, 0, SE, S], [0, 0, 0, 0]], np.uint8)
    c["branch_choice"] = (fdr, None, None, 1.0, np.array([[0, 11, 11, 11], [4, 5, 11, 11], [8, 9, 10, 11]]),
                          np.array([[0, 2 * r2, 3, 2], [0, 0, r2, 1], [0, 0, 0, 0]]), None,
                          np.array([[0, 0, 0, 1], [0, 0, r2, 2], [0, 0, 0, 3]]))
    return c
