"""Pure-numpy reference of descriptools_amd.flowpath and flowdir.d8_carved, independent of the kernels' schedule: the
upslope extreme by in-degree peeling for the acyclic part and a sweep to the fixed point over what peeling leaves
(D8 cycles), the downstream extreme by a gather with pointer doubling, both on the pair (value, -flat index) with NaN
skipped and -0.0 taken as +0.0.  Built on _watershed_ref.graph.

Shared by tests/test_flowpath_host.py (which checks it on hand-built cases with literal expected arrays and against a
plain walk per cell) and tests/test_gpu_flowpath.py (which holds the GPU to it cell for cell)."""
import numpy as np

from _watershed_ref import E, N, S, SE, W_, graph

NAN = np.float32(np.nan)


def _canon(values):
    v = np.array(values, np.float32).reshape(-1)
    v[v == 0] = 0.0  # -0.0 is taken as +0.0
    return v


def _better(kind, av, ai, bv, bi):
    """the pair (av, ai) beats (bv, bi): a value beats no value, then the order of `kind`, then the smaller index"""
    a, b = ~np.isnan(av), ~np.isnan(bv)
    with np.errstate(invalid="ignore"):
        strict = av > bv if kind == "max" else av < bv
        tie = av == bv
    return a & (~b | strict | (tie & (ai < bi)))


def _fold(kind, t, cv, ci, bv, bi):
    """fold the candidates (cv, ci) into the cells t of (bv, bi), any number per cell; True when something changed"""
    keep = ~np.isnan(cv)
    t, cv, ci = t[keep], cv[keep], ci[keep]
    if not t.size:
        return False
    o = np.lexsort((ci, -cv if kind == "max" else cv, t))  # per cell: the best candidate first
    t, cv, ci = t[o], cv[o], ci[o]
    first = np.r_[True, t[1:] != t[:-1]]
    t, cv, ci = t[first], cv[first], ci[first]
    g = _better(kind, cv, ci, bv[t], bi[t])
    bv[t[g]] = cv[g]
    bi[t[g]] = ci[g]
    return bool(g.any())


def _result(valid, bv, bi, shape):
    ok = valid & ~np.isnan(bv)
    return (np.where(ok, bv, NAN).astype(np.float32).reshape(shape),
            np.where(ok, bi, -100).astype(np.int64).reshape(shape))


def upslope(fdr, values, kind="max", dem=None):
    """(value float32, where int64) by the definition in descriptools_amd/flowpath.py"""
    fdr = np.asarray(fdr, np.uint8)
    n = fdr.size
    valid, succ, _ = graph(fdr, dem)
    v = _canon(values)
    bv = np.where(valid, v, NAN).astype(np.float32)
    bi = np.where(valid & ~np.isnan(v), np.arange(n, dtype=np.int64), -100)
    has = succ >= 0
    indeg = np.bincount(succ[has], minlength=n).astype(np.int64)
    done = np.zeros(n, bool)
    front = np.flatnonzero(valid & (indeg == 0))
    while front.size:
        done[front] = True
        f = front[succ[front] >= 0]
        t = succ[f]
        _fold(kind, t, bv[f], bi[f], bv, bi)
        np.subtract.at(indeg, t, 1)
        cand = np.unique(t)
        front = cand[(indeg[cand] == 0) & ~done[cand]]
    rest = np.flatnonzero(valid & ~done & has)  # D8 cycles: sweep until nothing changes
    while rest.size and _fold(kind, succ[rest], bv[rest].copy(), bi[rest].copy(), bv, bi):
        pass
    return _result(valid, bv, bi, fdr.shape)


def downstream(fdr, values, kind="max", dem=None, stop=None):
    """(value float32, where int64) by the definition in descriptools_amd/flowpath.py"""
    fdr = np.asarray(fdr, np.uint8)
    n = fdr.size
    valid, succ, _ = graph(fdr, dem)
    v = _canon(values)
    st = None if stop is None else (np.asarray(stop).reshape(-1) != 0)
    halt = valid & (succ < 0) if st is None else valid & st
    end = halt | (succ < 0) | ~valid
    ptr = np.where(end, np.arange(n, dtype=np.int64), succ)
    bv = np.where(valid, v, NAN).astype(np.float32)
    bi = np.where(valid & ~np.isnan(v), np.arange(n, dtype=np.int64), -100)
    rounds = 2
    while (1 << (rounds - 2)) < max(n, 1):
        rounds += 1
    for _ in range(rounds):
        g = _better(kind, bv[ptr], bi[ptr], bv, bi)
        bv = np.where(g, bv[ptr], bv)
        bi = np.where(g, bi[ptr], bi)
        ptr = ptr[ptr]
    good = valid if st is None else valid & halt[ptr]
    return _result(good, bv, bi, fdr.shape)


def carved(dem, px, max_cut=None):
    """(fdr, carved, filled) from oracle.condition_d8 and the upslope reference"""
    import oracle
    dem = np.asarray(dem, np.float32)
    fdr, filled = oracle.condition_d8(dem, px)
    low = upslope(fdr, dem, "min", dem)[0]
    if max_cut is not None and np.isfinite(max_cut):
        low = np.maximum(low, (filled.astype(np.float32) - np.float32(max_cut)).astype(np.float32))
    return fdr, np.where(dem <= -100, dem, low).astype(np.float32), filled


def walk(fdr, values, kind="max", dem=None, stop=None):
    """both folds by a plain walk from every cell, for small rasters: ((up value, up where), (down value, down where))"""
    fdr = np.asarray(fdr, np.uint8)
    n = fdr.size
    valid, succ, _ = graph(fdr, dem)
    v = _canon(values)
    st = None if stop is None else (np.asarray(stop).reshape(-1) != 0)

    def beats(a, b):  # cell a's value beats the best cell b (or None)
        if np.isnan(v[a]):
            return False
        if b is None:
            return True
        if v[a] != v[b]:
            return v[a] > v[b] if kind == "max" else v[a] < v[b]
        return a < b

    up = [None] * n
    dn = [None] * n
    for s in range(n):
        if not valid[s]:
            continue
        path, seen, c = [], set(), s
        while c >= 0 and c not in seen:
            seen.add(c)
            path.append(c)
            c = succ[c]
        for c in path:
            if beats(s, up[c]):
                up[c] = s
        best, met = None, st is None
        for c in path:
            if beats(c, best):
                best = c
            if st is not None and st[c]:
                met = True
                break
        dn[s] = best if met else None

    def arrays(w):
        val = np.array([NAN if c is None else v[c] for c in w], np.float32).reshape(fdr.shape)
        whr = np.array([-100 if c is None else c for c in w], np.int64).reshape(fdr.shape)
        return val, whr

    return arrays(up), arrays(dn)


def hand_cases():
    """name -> dict(fdr, dem, values, stop, kind, up=(value, where), dn=(value, where)): literal expected arrays; dn is
    taken with the case's stop (None: to the terminal)"""
    nan, inf = np.nan, np.inf
    f32 = lambda a: np.array(a, np.float32)
    i64 = lambda a: np.array(a, np.int64)
    c = {}
    # one row draining east to an outlet at the east edge
    c["row_to_edge"] = dict(
        fdr=np.array([[E, E, E, E]], np.uint8), dem=None, stop=None, kind="max", values=f32([[3, 1, 4, 2]]),
        up=(f32([[3, 3, 4, 4]]), i64([[0, 0, 2, 2]])), dn=(f32([[4, 4, 4, 2]]), i64([[2, 2, 2, 3]])))
    # three branches into (1,1); the 5 at (0,0) and the 5 at (0,2) tie: the smaller index wins
    c["two_branches_tie"] = dict(
        fdr=np.array([[SE, S, 8], [E, 0, 0]], np.uint8), dem=None, stop=None, kind="max",
        values=f32([[5, 2, 5], [1, 0, 7]]),
        up=(f32([[5, 2, 5], [1, 5, 7]]), i64([[0, 1, 2], [3, 0, 5]])),
        dn=(f32([[5, 2, 5], [1, 0, 7]]), i64([[0, 1, 2], [3, 4, 5]])))
    c["tie_along_a_path_min"] = dict(
        fdr=np.array([[E, E, 0]], np.uint8), dem=None, stop=None, kind="min", values=f32([[1, 1, 1]]),
        up=(f32([[1, 1, 1]]), i64([[0, 0, 0]])), dn=(f32([[1, 1, 1]]), i64([[0, 1, 2]])))
    # NaN is no value: cells with only NaN above (below) them have none
    c["nan_only_upstream"] = dict(
        fdr=np.array([[E, E, E, 0]], np.uint8), dem=None, stop=None, kind="max", values=f32([[nan, nan, 2, nan]]),
        up=(f32([[nan, nan, 2, 2]]), i64([[-100, -100, 2, 2]])),
        dn=(f32([[2, 2, 2, nan]]), i64([[2, 2, 2, -100]])))
    c["infinities_min"] = dict(
        fdr=np.array([[E, E, E]], np.uint8), dem=None, stop=None, kind="min", values=f32([[-inf, 5, inf]]),
        up=(f32([[-inf, -inf, -inf]]), i64([[0, 0, 0]])), dn=(f32([[-inf, 5, inf]]), i64([[0, 1, 2]])))
    c["infinities_max"] = dict(
        fdr=np.array([[E, E, E]], np.uint8), dem=None, stop=None, kind="max", values=f32([[-inf, 5, inf]]),
        up=(f32([[-inf, 5, inf]]), i64([[0, 1, 2]])), dn=(f32([[inf, inf, inf]]), i64([[2, 2, 2]])))
    # -0.0 is +0.0: it does not undercut the +0.0 before it, and comes back as +0.0
    c["negative_zero_min"] = dict(
        fdr=np.array([[E, 0]], np.uint8), dem=None, stop=None, kind="min", values=f32([[0.0, -0.0]]),
        up=(f32([[0, 0]]), i64([[0, 0]])), dn=(f32([[0, 0]]), i64([[0, 1]])))
    c["negative_zero_max"] = dict(
        fdr=np.array([[E, 0]], np.uint8), dem=None, stop=None, kind="max", values=f32([[-0.0, 0.0]]),
        up=(f32([[0, 0]]), i64([[0, 0]])), dn=(f32([[0, 0]]), i64([[0, 1]])))
    # (0,0) -> SE (1,1) -> E (1,2), which points into nodata (1,3): a terminal
    c["diagonal_into_nodata"] = dict(
        fdr=np.array([[SE, 0, 0, 0], [0, E, E, E]], np.uint8), dem=f32([[1, 1, 1, 1], [1, 1, 1, -100]]), stop=None,
        kind="max", values=f32([[9, 1, 2, 3], [4, 5, 6, 7]]),
        up=(f32([[9, 1, 2, 3], [4, 9, 9, nan]]), i64([[0, 1, 2, 3], [4, 0, 0, -100]])),
        dn=(f32([[9, 1, 2, 3], [4, 6, 6, nan]]), i64([[0, 1, 2, 3], [4, 6, 6, -100]])))
    # a 2 x 2 cycle with the tributary (1,2): every cycle cell gets the extreme over the cycle and what reaches it
    c["cycle_with_tributary"] = dict(
        fdr=np.array([[E, S, 0], [N, W_, W_]], np.uint8), dem=None, stop=None, kind="max",
        values=f32([[1, 2, 3], [4, 5, 9]]),
        up=(f32([[9, 9, 3], [9, 9, 9]]), i64([[5, 5, 2], [5, 5, 5]])),
        dn=(f32([[5, 5, 3], [5, 5, 9]]), i64([[4, 4, 2], [4, 4, 5]])))
    c["cycle_with_tributary_min"] = dict(
        fdr=np.array([[E, S, 0], [N, W_, W_]], np.uint8), dem=None, stop=None, kind="min",
        values=f32([[4, 2, 3], [4, 5, 1]]),
        up=(f32([[1, 1, 3], [1, 1, 1]]), i64([[5, 5, 2], [5, 5, 5]])),
        dn=(f32([[2, 2, 3], [2, 2, 1]]), i64([[1, 1, 2], [1, 1, 5]])))
    # a stop cell on a cycle stops it; (1,2) is a terminal that meets no stop cell
    c["stop_cell_on_cycle"] = dict(
        fdr=np.array([[E, S, 0], [N, W_, 0]], np.uint8), dem=None, stop=np.array([[0, 1, 1], [0, 0, 0]], np.int32),
        kind="max", values=f32([[1, 2, 3], [7, 5, 6]]),
        up=(f32([[7, 7, 3], [7, 7, 6]]), i64([[3, 3, 2], [3, 3, 5]])),
        dn=(f32([[2, 2, 3], [7, 7, nan]]), i64([[1, 1, 2], [3, 3, -100]])))
    # a cycle without a stop cell on it, with a stop raster: no value
    c["cycle_without_stop"] = dict(
        fdr=np.array([[E, S, 0], [N, W_, W_]], np.uint8), dem=None, stop=np.array([[0, 0, 1], [0, 0, 0]], bool),
        kind="max", values=f32([[1, 2, 3], [4, 5, 9]]),
        up=(f32([[9, 9, 3], [9, 9, 9]]), i64([[5, 5, 2], [5, 5, 5]])),
        dn=(f32([[nan, nan, 3], [nan, nan, nan]]), i64([[-100, -100, 2], [-100, -100, -100]])))
    # a stop cell on nodata is ignored: the cell above it is a terminal without a stop cell
    c["stop_on_nodata"] = dict(
        fdr=np.array([[S], [S], [0]], np.uint8), dem=f32([[1], [-200], [1]]), stop=np.array([[0], [1], [1]], np.uint8),
        kind="max", values=f32([[4], [5], [6]]),
        up=(f32([[4], [nan], [6]]), i64([[0], [-100], [2]])),
        dn=(f32([[nan], [nan], [6]]), i64([[-100], [-100], [2]])))
    # the path below the stop cell ends at a terminal without meeting another
    c["terminal_without_stop"] = dict(
        fdr=np.array([[E, E, E, E, 0]], np.uint8), dem=None, stop=np.array([[0, 1, 0, 0, 0]], np.int64), kind="max",
        values=f32([[1, 2, 3, 4, 5]]),
        up=(f32([[1, 2, 3, 4, 5]]), i64([[0, 1, 2, 3, 4]])),
        dn=(f32([[2, 2, nan, nan, nan]]), i64([[1, 1, -100, -100, -100]])))
    return c
